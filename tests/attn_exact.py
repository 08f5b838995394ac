"""Exact-operand cases for the attention kernels: attention.hip (attn_f16_v0 and attn_f32_small), attention_v1.hip,
attention_v3.hip, attention_v5.hip and attention_short.hip, with the steps they share in attn_common.h, behind
ovmr_debug_attention and ovmr_debug_attention_q.  numpy and torch on the CPU, no library: shared by
test_hip_attn_exact.py (GPU), test_attn_exact_cpu.py (which checks this builder) and test_attn_route_cpu.py (which
holds the library's routing function to route() below and checks that the case table reaches every kernel).

THE METHOD (gemm_exact.py carried over to softmax)

Scores have TWO levels.  A key carries a code u_c in {+-1}^64 as its K row 4 u_c, and a query that addresses code c
has the Q row 4 u_c.  The raw score is the integer 1024 - 32 d at Hamming distance d, exact in the matrix pipe in
any order.  The drawn codes are at distance >= 8 from each other (asserted), so under the kernels' scale of 1/8
every key that is not addressed lies at least 32 below the match in the natural-log domain: its P is 0 in fp16
(e^-32 = 2^-46) and its share of an fp32 row sum or accumulator is below 2^-25 of a matching key's.

Keys that share a code have bit-identical scores whatever the summation order.  1024 * (0.125 log2 e) is exact in
fp32 (a power of two times the constant), so their P is exactly 1 against any reference maximum a kernel can hold
once it has seen one of them.  The output row is then the plain mean of the V rows of the addressed group: ONE
fp16 bit pattern, computed here with integer / `fractions` arithmetic and no softmax.

V rows are non-zero integers in [-15, 15], drawn per (sequence, head, key), all rows distinct.  Codes, groups and
permutations differ per (sequence, head): a mix-up of heads or sequences changes the result.

The expected mean sum / count (count in 1, 2, 3, 4) is rounded to fp16 exactly.  It is asserted that none lies
within relative 2^-20 of a rounding tie.  Halves and quarters of |sum| <= 60 are fp16 values; a third has the
mantissa tail 0101.. or 1010..: a sixth of a step from the tie, relative 2^-13.6.

THE CASES

  "onehot"   groups of one key; query i addresses key pi(i), pi not the identity.
  "groups"   sizes 1, 2, 4 and, fp16 only, 3.  Members are placed on key 0, key L - 1, both sides of every 16-key
             boundary (the 32- and 64-key boundaries among them), the tail block, the last full block, the first
             and last key of a lane's quartet: the PLACEMENT CLASSES of key_classes().
  "causal"   query i addresses the group of key i: the members > i score 1024 and must be masked.
  "uniform"  Q = 0, every valid key weighs the same.  v[k][d] = bit d of k for d < 10, k mod 7 / 5 / 3 from column
             10 on, the columns rotated by the (sequence, head) index.  Expected sum / n with n = L.
  "ucausal"  the uniform case under the mask: n = q + 1.
  "three"    the one path two levels cannot reach, a tolerance case: see three_level().

"Every group is addressed in every query tile" is read as: every group is addressed by some query, and every full
16-row query tile addresses every placement class and every group size.  A length has up to about 250 groups and
a tile 16 rows, so no tile can address every group; the ragged last tile addresses what its rows allow.

TWO DEVIATIONS, both named where they act

1. One sign per (group, column).  The members of a group carry ONE SIGN PER COLUMN, so that no partial sum of a
   column cancels.  The e^-32 shares are negligible against a sum of magnitude >= 1, not against 0: where a column
   of a group sums to 0 the fp64 reference itself returns about +-1e-14, not 0, and a kernel returns more than
   that.  Observed with mixed signs under variant 0 at L = 127 .. 144: -2^-24 .. -2^-22 in about 10 of 73 000
   elements, all of them where 0 was expected, all negative.  A zero has no relative margin for a bit comparison,
   so the builder draws no cancelling sums.  Sums whose exact value is 0 are therefore tested nowhere.

   What fits the observation (a fit, not a finding): the flash kernels hold o = alpha * (what the far keys of the
   earlier blocks left), a tiny number, when the first member's block arrives.  A matrix pipe that aligns C and
   the products to the largest exponent and truncates toward -inf (v_mfma_f32_16x16x32_f16, attention.hip:133)
   would charge a tiny negative C one unit of the adder's last place, 2^-24 of the largest addend.  For the first
   element found: -10 + 5 - tiny = -5 - 2^-21, the next step's + 2 + 3 leaves -2^-21, and the division by 4 gives
   the -2^-23 that was read.  A CPU emulation of variant 0 with round-to-nearest sums gives -0 there.  With one
   sign per column such a unit is at most 2^-23 of the final sum and occurs once per row (later steps add integers
   and exact zeros): the tie margin holds it.

2. NEAR_TIES: two quotients of the uniform case at L = 273 cannot keep 2^-20 and are held to 2^-22 (see there).
"""
import functools
import itertools
from fractions import Fraction
from typing import NamedTuple

import numpy as np
import torch

ATTN_VARIANTS = (0, 1, 3, 5)
B, H = 3, 3                 # B * H = 9: the last XCD slot of variants 1 and 5 runs through its `bh >= nBH` return
SENTINEL = 0x5A5A
SENTINEL32 = 0x5A5A5A5A
PAD_ROWS = 16
MIN_DISTANCE = 8
TIE_MARGIN = Fraction(1, 1 << 20)       # no expected value within this relative distance of an fp16 rounding tie
# One mantissa of the case table cannot keep 2^-20: 17 / 273 and 136 / 273 = 8 * 17 / 273 (bits 8 and 3 of k in the
# uniform case at L = 273) lie 2^-20.09 from a tie.  What the margin has to cover is the kernels' own arithmetic on
# an exact numerator o and an exact row sum l = n: inv = fl(1 / l), within 2^-24 relative where the divide is
# correctly rounded and within 2^-23 where it is a reciprocal good to one unit in the last place, and fl(o * inv),
# within 2^-24.  Together at most 1.5 * 2^-23, whichever divide the compiler emits: under the 2^-22 these two
# quotients are held to.  All others keep 2^-20.
NEAR_TIES = {Fraction(17, 273): Fraction(1, 1 << 22), Fraction(136, 273): Fraction(1, 1 << 22)}

# Which kernel a length runs under a variant: route() below, held to the library's routing function by test_attn_route_cpu.py.
SHORT_L = (1, 5, 16, 17, 32, 33)                        # <= 32: the short kernel under every variant but 0; 33: just past it
MID_L = (63, 64, 65, 77, 127, 128, 129, 144, 145)       # 128: where variant 1 starts; 144 / 145: its tail of 16 / 17 keys (peeled or not)
SINGLE_L = (192, 193, 197, 208, 209)                    # 193 .. 208: the single-pass kernel under variant 3, and both sides of it
LONG_L = (256, 257, 272, 273, 320, 321, 336, 337, 577)  # >= 256: variant 5's kernel; 272 / 273: its peel boundary; 320 .. 337: variant 1's
Q_L, Q_LQ = (197, 257, 577), (1, 16, 17, 33)
F32_L, F32_UNIFORM_L = (6, 18, 66, 127, 128), (16, 64, 128)
THREE_L = (197, 257, 577)


class Case(NamedTuple):
    kind: str                   # "onehot" | "groups" | "causal" | "uniform" | "ucausal" (uniform under the mask)
    L: int
    variants: tuple             # () for the fp32 kernel
    f32: bool = False

    @property
    def causal(self):
        return int(self.kind in ("causal", "ucausal"))

    @property
    def id(self):
        return f"{'f32-' if self.f32 else ''}{self.kind}-L{self.L}"


def _cases():
    out = []
    for L in SHORT_L + MID_L + SINGLE_L + LONG_L:
        v = (0, 1, 3) if L < 192 else ATTN_VARIANTS
        out += [Case(k, L, v) for k in ("onehot", "groups", "uniform")]
        if L < 192:
            out += [Case(k, L, v) for k in ("causal", "ucausal")]
        elif L == 197:
            out += [Case(k, L, (0, 1)) for k in ("causal", "ucausal")]
    out += [Case(k, L, (), True) for L in F32_L for k in ("onehot", "groups")]
    out += [Case("uniform", L, (), True) for L in F32_UNIFORM_L]
    return out


CASES = _cases()


# ---- which kernel runs ---------------------------------------------------------------------------------------

V0, V1, SHORT, V3, V5 = 0, 1, 2, 3, 5       # attn_f16_v0, attn_f16_v1, attn_f16_short, attn_f16_v3, attn_f16_v5


def route(variant, L, Lq, causal):
    """The kernel launch_attention_f16_q ran for (variant, L, Lq <= L, causal) when each launcher still tested its own
    shape and declined with -100: restated from that chain, step for step, not from the library's routing function."""
    def short_declines():       # one group, first row 0: the launcher declined a group longer than 32 tokens
        return L < 1 or L > 32

    def v3_declines():
        return bool(causal) or Lq != L or L <= 192 or L > 208

    def v5_declines():
        return bool(causal) or L < 256 or Lq < 32

    if variant >= 1 and Lq == L and L <= 32:
        if not short_declines():
            return SHORT
    if variant == 4:
        variant = 3
    if variant == 3:
        if not v3_declines():
            return V3
        if not v5_declines():
            return V5
        variant = 1
    if variant == 5:
        if not v5_declines():
            return V5
        variant = 1
    if variant == 1 and L >= 128:
        return V1               # variant 1's launcher declined no shape
    return V0


# ---- codes ---------------------------------------------------------------------------------------------------

def min_distance(u):
    """Smallest pairwise Hamming distance of the rows of u in {+-1}^64 (64 for a single row)."""
    d = (64 - u.astype(np.int32) @ u.astype(np.int32).T) // 2
    d[np.diag_indices(len(u))] = 64
    return int(d.min())


def draw_codes(n, seed):
    """n sign vectors [n, 64] int8 at pairwise distance >= MIN_DISTANCE: redrawn with the next seed otherwise."""
    for s in itertools.count(seed):
        u = (np.random.default_rng(s).integers(0, 2, (n, 64)) * 2 - 1).astype(np.int8)
        if min_distance(u) >= MIN_DISTANCE:
            return u


# ---- exact rounding ------------------------------------------------------------------------------------------

def round_half(fr):
    """(the fp16 value nearest to the Fraction fr, ties to even, as a float;
    the relative distance of fr to the nearest rounding tie)."""
    if fr == 0:
        return 0.0, Fraction(1)
    a = abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    e = max(e - 1 if Fraction(2) ** e > a else e, -14)
    ulp = Fraction(2) ** (e - 10)
    q = a / ulp
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    val = float(n * ulp)
    assert val <= 65504.0
    return (val if fr > 0 else -val), abs(rem - Fraction(1, 2)) * ulp / a


def quotients_fp16(num, den):
    """num / den (int64 arrays of one shape, den > 0) rounded to fp16 exactly, one Fraction per distinct pair.
    Asserts the tie margin."""
    num, den = np.broadcast_arrays(np.asarray(num, np.int64), np.asarray(den, np.int64))
    assert int(den.min()) > 0 and int(np.abs(num).max()) < (1 << 20) and int(den.max()) < (1 << 20)
    key = (num + (1 << 20)) * (1 << 21) + den
    uniq, inv = np.unique(key.ravel(), return_inverse=True)
    vals = np.empty(len(uniq), np.float64)
    for i, k in enumerate(uniq.tolist()):
        fr = Fraction((k >> 21) - (1 << 20), k & ((1 << 21) - 1))
        vals[i], tie = round_half(fr)
        margin = NEAR_TIES.get(fr, TIE_MARGIN)
        assert tie >= margin, f"{fr} lies within relative {float(tie):.3e} of an fp16 rounding tie"
    return torch.from_numpy(vals[inv].reshape(num.shape)).half()


# ---- placement -----------------------------------------------------------------------------------------------

def key_classes(k, L):
    """The placement classes key k of L belongs to (module docstring).  A group holds the union over its members."""
    c = set()
    if k == 0:
        c.add("key0")
    if k == L - 1:
        c.add("last")
    for m in (16, 32, 64):
        if k % m == m - 1 and k + 1 < L:
            c.add(f"below{m}")
        if k % m == 0 and k > 0:
            c.add(f"above{m}")
    if L >= 64 and k // 64 == L // 64 - 1:
        c.add("lastfull")
    if L > 64 and L % 64 and k // 64 == L // 64:
        c.add("tail")
    if k % 4 == 0:
        c.add("quad0")
    if k % 4 == 3:
        c.add("quad3")
    return c


def group_classes(g, L):
    return set().union(*(key_classes(k, L) for k in g)) | {f"size{len(g)}"}


def _split(keys, sizes):
    """keys cut into groups of allowed sizes, the largest first."""
    out = []
    while keys:
        n = max(s for s in sizes if s <= len(keys))
        out.append(keys[:n])
        keys = keys[n:]
    return out


def partition(L, rng, sizes):
    """Every key of range(L) in exactly one group (list of sorted key lists).  Placed on purpose:
      * one group with key 0, key L - 1, the first key of the tail block and the last key of the last full block;
      * the keys 16 j - 1 and 16 j of every boundary together in one group of 2, 4 or 3 keys, filled up with
        keys from anywhere;
      * the rest in shuffled groups whose sizes cycle through `sizes`."""
    used = np.zeros(L, bool)
    special = {0, L - 1}
    for b in range(16, L, 16):
        special |= {b - 1, b}
    filler = [int(k) for k in rng.permutation(L) if int(k) not in special]
    groups = []

    def close(keys):
        for g in _split(keys, sizes):
            used[g] = True
            groups.append(sorted(g))

    def emit(keys, want):
        """The placed keys that are still free, filled up to `want` keys and then to an allowed size."""
        keys = [k for k in dict.fromkeys(keys) if 0 <= k < L and not used[k]]
        while filler and len(keys) < want:
            keys.append(filler.pop())
        while filler and keys and len(keys) not in sizes:
            keys.append(filler.pop())
        close(keys)

    t0 = (L - 1) // 64 * 64                         # first key of the last (tail or full) block
    emit([0, L - 1] + ([t0, t0 - 1] if t0 else []), 2)
    multi = [s for s in sizes if s > 1]
    for j, b in enumerate(range(16, L, 16)):
        emit([b - 1, b], multi[j % len(multi)])
    rest = [k for k in filler if not used[k]]
    filler.clear()
    i = 0
    while rest:
        n = min(sizes[i % len(sizes)], len(rest))
        close(rest[:n])
        rest = rest[n:]
        i += 1
    assert used.all() and sum(len(g) for g in groups) == L
    return groups


def address(groups, L, rng):
    """Group index per query [L].  In every full 16-row query tile the rows address groups that together hold every
    placement class and every group size there is: a greedy cover that prefers groups nobody addressed yet.  The
    other rows address the groups not yet addressed.  The rows of a tile come in shuffled order.  Every group is
    addressed (asserted)."""
    cls = [group_classes(g, L) for g in groups]
    every = set().union(*cls)
    seen = np.zeros(len(groups), bool)
    order = [int(i) for i in rng.permutation(len(groups))]      # least recently addressed first
    a = np.zeros(L, np.int64)

    def take(i, picks):
        picks.append(i)
        seen[i] = True
        order.remove(i)
        order.append(i)

    for t0 in range(0, L, 16):
        rows = min(16, L - t0)
        picks, need = [], set(every)
        while need and len(picks) < rows:
            best = max(order, key=lambda i: (len(cls[i] & need), not seen[i]))
            if not cls[best] & need:
                break
            take(best, picks)
            need -= cls[best]
        assert rows < 16 or not need, f"tile {t0 // 16} of L = {L} misses {need}"
        while len(picks) < rows:
            fresh = [i for i in order if not seen[i]]
            take(fresh[0] if fresh else order[0], picks)
        a[t0:t0 + rows] = np.asarray(picks)[rng.permutation(rows)]
    assert seen.all(), f"L = {L}: {int((~seen).sum())} groups are addressed by no query"
    return a


def permutation(L, rng, bh):
    """pi [L], not the identity for L > 1.  The first queries address the keys at the edges -- L - 1, the first key
    of the tail block, the last of the last full block, 0, the keys around 16 / 32 / 64 -- starting at another one
    per (sequence, head); the rest is shuffled."""
    t0 = (L - 1) // 64 * 64
    edge = [k for k in dict.fromkeys([L - 1, t0, t0 - 1, 0, 63, 64, 15, 16, 31, 32, L - 2, 3, 4]) if 0 <= k < L]
    edge = edge[bh % len(edge):] + edge[:bh % len(edge)]
    rest = [int(k) for k in rng.permutation(L) if int(k) not in edge]
    pi = np.asarray(edge + rest, np.int64)
    if L > 1 and (pi == np.arange(L)).all():
        pi = np.roll(pi, 1)
    return pi


# ---- the operands --------------------------------------------------------------------------------------------

class Built(NamedTuple):
    qkv: torch.Tensor           # [B * L, 3 * H * 64] fp16 (fp32 for the fp32 kernel)
    want: torch.Tensor          # [B * L, H * 64] fp16 (fp32): the expected output
    heads: list                 # per (b, h): dict(groups, addr, codes)


def pack(q, k, v, dtype):
    """q, k, v [B, H, L, 64] -> qkv [B * L, 3 * H * 64]."""
    b, h, L, _ = q.shape
    t = torch.from_numpy(np.stack([q, k, v])).permute(1, 3, 0, 2, 4).reshape(b * L, 3 * h * 64)
    return t.to(dtype).contiguous()


def unpack_rows(x):
    """[B, H, L, 64] -> [B * L, H * 64]."""
    b, h, L, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(b * L, h * 64).contiguous()


def uniform_values(L, bh):
    """v [L, 64] of the uniform case: bit d of k for d < 10, k mod (7, 5, 3)[(d - 10) % 3] from column 10 on;
    columns rotated by bh."""
    k = np.arange(L, dtype=np.int64)[:, None]
    d = np.arange(64, dtype=np.int64)[None, :]
    mod = np.asarray([7, 5, 3], np.int64)[(np.maximum(d, 10) - 10) % 3]
    v = np.where(d < 10, (k >> np.minimum(d, 9)) & 1, k % mod)
    return np.roll(v, bh, axis=1)


def _group_of_key(groups, L):
    of_key = np.empty(L, np.int64)
    for gi, g in enumerate(groups):
        of_key[g] = gi
    return of_key


KIND_SEED = {"onehot": 1, "groups": 2, "causal": 3, "uniform": 4, "ucausal": 5}


@functools.lru_cache(maxsize=4)
def build(kind, L, f32=False, b=B, h=H):
    sizes = (1, 2, 4) if f32 else (1, 2, 4, 3)
    causal = kind in ("causal", "ucausal")
    q, k, v = (np.zeros((b, h, L, 64), np.int64) for _ in range(3))
    want = torch.empty((b, h, L, 64), dtype=torch.float32 if f32 else torch.float16)
    heads = []
    tri = np.tril(np.ones((L, L), bool)) if causal else np.ones((L, L), bool)       # [query, key]: who may be seen
    for bh in range(b * h):
        seed = 1000 * L + 10 * bh + KIND_SEED[kind] + (7 if f32 else 0)
        rng = np.random.default_rng(seed)
        if kind in ("uniform", "ucausal"):
            codes = draw_codes(L, seed)
            kk, vv = 4 * codes.astype(np.int64), uniform_values(L, bh)
            groups, addr = [list(range(L))], np.zeros(L, np.int64)
            num, den = tri.astype(np.int64) @ vv, tri.sum(1)[:, None]
        else:
            if kind == "onehot":
                groups, addr = [[i] for i in range(L)], permutation(L, rng, bh)
            else:
                groups = partition(L, rng, sizes)
                addr = _group_of_key(groups, L) if causal else address(groups, L, rng)
            codes = draw_codes(len(groups), seed)
            of_key = _group_of_key(groups, L)
            kk = 4 * codes[of_key].astype(np.int64)
            q[bh // h, bh % h] = 4 * codes[addr].astype(np.int64)
            mag = rng.integers(1, 16, (L, 64))
            sign = rng.integers(0, 2, (len(groups), 64))[of_key]        # one sign per (group, column): deviation 1
            vv = mag * (2 * sign - 1)
            assert len(np.unique(vv, axis=0)) == L, "two keys with the same V row"
            member = (of_key[None, :] == addr[:, None]) & tri           # [query, key]
            num, den = member.astype(np.int64) @ vv, member.sum(1)[:, None]
        k[bh // h, bh % h], v[bh // h, bh % h] = kk, vv
        if f32:
            x = num.astype(np.float64) / den
            assert (np.log2(den) % 1 == 0).all(), "a group size that is no power of two"
            assert (x.astype(np.float32).astype(np.float64) == x).all(), "an expected value that is not an fp32 value"
            want[bh // h, bh % h] = torch.from_numpy(x.astype(np.float32))
        else:
            want[bh // h, bh % h] = quotients_fp16(num, den)
        heads.append(dict(groups=groups, addr=addr, codes=codes))
    dtype = torch.float32 if f32 else torch.float16
    qkv = pack(q, k, v, dtype)
    assert torch.equal(qkv.double(), pack(q, k, v, torch.float64))      # every operand is an fp16 value
    return Built(qkv, unpack_rows(want), heads)


# ---- the lazy reference: three score levels ------------------------------------------------------------------

ORDERS = list(itertools.permutations(range(3)))     # which of three ascending key blocks holds distance 0, 1, 2


class Three(NamedTuple):
    qkv: torch.Tensor           # [B * L, 3 * H * 64] fp16
    tiles: list                 # per (b, h), per 32-row query tile: (order 0 .. 5, or 6: one block; blocks; keys)


def _first_triple(combos, start, free):
    """The first block triple, from combos[start] on and cyclically, all of whose blocks still have a free key."""
    for i in range(len(combos)):
        c = combos[(start + i) % len(combos)]
        if all(free[x] for x in c):
            return c
    raise AssertionError("no block triple with free keys left")


def _first_block(nb, start, free):
    """The first key block, from `start` on and cyclically, with three free keys."""
    for i in range(nb):
        x = (start + i) % nb
        if len(free[x]) >= 3:
            return x
    raise AssertionError("no block with three free keys left")


@functools.lru_cache(maxsize=2)
def three_level(L, b=B, h=H):
    """Rows whose reference maximum is stale.

    Variants 1 and 5 move the maximum they take exponentials against only when a block maximum exceeds it by more
    than 8 in the log2 domain, and the test is a ballot over the wave: a reference stays stale only if no row of
    the wave's query tile asks for a move in that block.  So all rows of a 32-row query tile (variant 5's tile,
    two of variant 1's) address codes whose three near keys lie in the SAME key blocks in the same order:
      * the key at Hamming distance 0: raw score 1024;
      * the key at distance 1: 992, 5.77 below in the log2 domain, under the threshold.  The reference stays and
        P of the match is about 54;
      * the key at distance 2: 960, 11.5 below.  The reference moves and alpha is applied.
    Tile t of (sequence, head) bh takes order (t + bh) mod 7: the six orders over three different key blocks, then
    all three keys in one block.  The block triples cycle, those with block 0 and the last block first.  A tile
    has up to two codes, and its rows alternate between them.  Every other key has a far code (distance >=
    MIN_DISTANCE from every query's code).  V: fp16 values in [1, 2)."""
    nb = (L + 63) // 64
    q, k = (np.zeros((b, h, L, 64), np.int64) for _ in range(2))
    v = np.zeros((b, h, L, 64), np.float64)
    combos = sorted(itertools.combinations(range(nb), 3), key=lambda c: -((0 in c) + (nb - 1 in c)))
    tiles_all = []
    for bh in range(b * h):
        seed = 5000 * L + bh
        rng = np.random.default_rng(seed)
        nt = (L + 31) // 32
        codes = draw_codes(L + 2 * nt, seed)
        kk = 4 * codes[:L].astype(np.int64)
        free = []                                   # per key block: its keys not yet given a near code, shuffled
        for blk in range(nb):
            free.append([int(x) for x in rng.permutation(np.arange(blk * 64, min(L, blk * 64 + 64)))])
        tiles = []
        for t in range(nt):
            order = (t + bh) % 7
            if order < 6:
                blocks = _first_triple(combos, t, free)
                ncodes = 2 if all(len(free[x]) >= 2 for x in blocks) else 1
                place = ORDERS[order]
            else:
                blk = _first_block(nb, t, free)
                blocks = (blk, blk, blk)
                ncodes = 2 if len(free[blk]) >= 6 else 1
                place = (0, 1, 2)
            keys = []
            for c in range(ncodes):
                u = codes[L + 2 * t + c].astype(np.int64)
                mine = []
                for dist in range(3):
                    key = free[blocks[place[dist]]].pop()
                    near = u.copy()
                    near[rng.permutation(64)[:dist]] *= -1
                    kk[key] = 4 * near
                    mine.append(key)
                keys.append(mine)
                rows = np.arange(t * 32 + c, min(L, t * 32 + 32), ncodes)
                q[bh // h, bh % h, rows] = 4 * u
            tiles.append((order, blocks, keys))
        k[bh // h, bh % h] = kk
        v[bh // h, bh % h] = 1.0 + rng.integers(0, 1024, (L, 64)) / 1024.0
        tiles_all.append(tiles)
    return Three(pack(q.astype(np.float64), k.astype(np.float64), v, torch.float16), tiles_all)


# ---- the comparator ------------------------------------------------------------------------------------------

def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def sentinel_buffer(rows, cols, dtype, device="cpu"):
    t = torch.empty((rows, cols), dtype=dtype, device=device)
    bits(t).fill_(SENTINEL32 if dtype == torch.float32 else SENTINEL)
    return t


def untouched(t):
    return bool((bits(t) == (SENTINEL32 if t.dtype == torch.float32 else SENTINEL)).all())


def mismatch(got, want, rows_per_seq):
    """None if got == want element for element (torch.equal: +0 and -0 are one value, a NaN equals nothing).
    Else: how many elements differ, the first one's (sequence, query, head, column), its query tile and row in it,
    and both values."""
    assert got.shape == want.shape and got.dtype == want.dtype, \
        f"{tuple(got.shape)} {got.dtype} against {tuple(want.shape)} {want.dtype}"
    if torch.equal(got, want):
        return None
    bad = ~(got == want)
    r, c = (int(i) for i in bad.nonzero()[0])
    seq, qi = divmod(r, rows_per_seq)
    qrows = sorted({int(i) % rows_per_seq for i in bad.any(1).nonzero().flatten()})
    more = " ..." if len(qrows) > 12 else ""
    return (f"{int(bad.sum())} of {bad.numel()} elements differ, in {int(bad.any(1).sum())} rows "
            f"(queries {qrows[:12]}{more}); first at sequence {seq}, query {qi} "
            f"(row {qi % 16} of 16-row tile {qi // 16}), head {c // 64}, column {c % 64}: "
            f"got {float(got[r, c])!r}, want {float(want[r, c])!r}")
