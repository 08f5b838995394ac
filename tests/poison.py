"""Poisoned memory: the fills and the guarded allocator behind test_poison_cpu.py and test_hip_poison.py.  Plain torch, importable
without a GPU.

The property held.  The result of a call is a function of that call's inputs and weights, and of nothing else that happens to lie in
memory: every pass writes what it later reads, every over-read is clamped or selected away, nothing is assumed zero.  The exact suites
hand every kernel clean memory -- zeroed operands with zero slack, a workspace fresh from the allocator or holding the finite leftovers
of a similar call -- so a kernel can lean on a value it never wrote and stay green.  Here the same call runs over four different
contents of everything it did not write, and the outputs are compared as bit patterns.

FILLS: four 32-bit patterns, and what each is when a kernel reads it as

    name    pattern      fp16 (both halves)   fp32                  int32
    zero    0x00000000   +0                   +0                    0
    nan16   0x7E007E00   quiet NaN            finite, about 2^125   large positive
    ones    0xFFFFFFFF   NaN                  NaN                   -1
    big     0x7BFF7BFF   65504                finite, about 2^120   large positive

All four are needed.  A NaN never wins a `>` comparison, so a stale row that only VOTES (the wave-wide ballot of a lazily moved softmax
reference) shows under `big` and not under the NaN fills; a tail masked by multiplying with zero shows under NaN and not under `big`
(65504 * 0 = 0); an accumulator assumed zero shows under every non-zero fill.  test_poison_cpu.py asserts exactly this detection matrix
on three planted defects.

Arena(fill, device, guard): take(elems, kind) hands out a flat view with at least `guard` elements of the fill in front of the operand
and `guard` behind it; the operand's own elements start as the fill too.  The first element is 256-byte aligned (the kernels route on
16-byte alignment: a guard must not change the route).  Integer buffers (ids, index, labels, offset tables) are filled with 0 under
`zero` and with 1 under every other fill: every kernel can index with those values, so an over-read shows in the bits and never as a
wild address.  place(t) is take + copy, place_all a dict of them (weights guarded once and shared by several replays).  intact() says
whether every guard still holds its fill: a stray store shows there.
"""
import torch

FILLS = {"zero": 0x00000000, "nan16": 0x7E007E00, "ones": 0xFFFFFFFF, "big": 0x7BFF7BFF}
KINDS = {"f16": torch.float16, "f32": torch.float32, "i32": torch.int32, "i64": torch.int64}
ALIGN = 256
ROW_TILE = 256                          # the tallest row tile of any kernel (the 256-row GEMM family)


def _i32(pattern):
    """The pattern as the int32 with those bits."""
    return pattern - (1 << 32) if pattern >= 1 << 31 else pattern


def as_read(pattern):
    """What a kernel reads from memory filled with the pattern: {"f16": (low half, high half), "f32": value, "i32": value}."""
    w = torch.tensor([_i32(pattern)], dtype=torch.int32)
    h = w.view(torch.float16)
    return {"f16": (float(h[0]), float(h[1])), "f32": float(w.view(torch.float32)[0]), "i32": int(w[0])}


def int_fill(fill):
    """The value integer buffers and their guards hold under the fill: an index every kernel can use."""
    return 0 if FILLS[fill] == 0 else 1


def kind_of(t):
    return {v: k for k, v in KINDS.items()}[t.dtype]


def fill_(t, fill):
    """t (any kind of KINDS, contiguous) set to the fill in place: the pattern's bits for floating point, int_fill for integers."""
    if t.numel() == 0:
        return t
    if not t.is_floating_point():
        return t.fill_(int_fill(fill))
    p = FILLS[fill]
    if t.dtype == torch.float16:
        t.view(torch.int16).fill_((p & 0xFFFF) - (1 << 16) if p & 0x8000 else p & 0xFFFF)     # both halves of every pattern are equal
    else:
        t.view(torch.int32).fill_(_i32(p))
    return t


def guard_elems(widest_row):
    """One row tile of the widest row a case uses: the farthest any tile of any kernel can reach past, or in front of, an operand."""
    return ROW_TILE * int(widest_row)


class Arena:
    """Guarded allocations under one fill.  Every take() is an allocation of its own (so a guard is never another operand's data):
    [slack to alignment][guard][operand][guard], all of it the fill before the operand is handed out."""

    def __init__(self, fill, device="cpu", guard=guard_elems(16)):
        assert fill in FILLS and guard >= 1
        self.fill, self.device, self.guard, self.keep = fill, device, int(guard), []

    def take(self, elems, kind="f16"):
        dt = KINDS[kind]
        es = torch.empty((), dtype=dt).element_size()
        g = (self.guard * es + ALIGN - 1) // ALIGN * ALIGN                       # bytes of one guard, whole alignment units
        raw = torch.empty(g + ALIGN + (elems * es + 7) // 8 * 8 + g, dtype=torch.uint8, device=self.device)
        start = (-(raw.data_ptr() + g)) % ALIGN + g                              # first byte of the operand: aligned, at least g in
        assert raw.data_ptr() % 8 == 0 and start % 8 == 0
        fill_(raw.view(dt), self.fill)
        view = raw[start:start + elems * es].view(dt)
        assert elems == 0 or view.data_ptr() % ALIGN == 0
        self.keep.append((raw, start, elems * es, dt))
        return view

    def place(self, t):
        """A guarded copy of t on the arena's device: same dtype, same shape, contiguous."""
        v = self.take(t.numel(), kind_of(t))
        v.copy_(t.reshape(-1))
        return v.view(t.shape)

    def place_all(self, tensors):
        """name -> guarded copy, as a Placed: engine_replay.Hooks takes it as weights that are guarded already (under this arena's fill)."""
        out = Placed((k, self.place(v)) for k, v in tensors.items())
        out.arena = self
        return out

    def guards(self, i):
        """(front, behind) of the i-th allocation, in its dtype: every element must still be the fill."""
        raw, start, nbytes, dt = self.keep[i]
        return raw[:start].view(dt), raw[start + nbytes:].view(dt)                # (both a whole number of elements: 8-byte units)

    def intact(self):
        """True where no guard has been written to (bit patterns, so a NaN fill compares equal to itself)."""
        bad = None
        for i, (_, _, _, dt) in enumerate(self.keep):
            want = fill_(torch.empty(1, dtype=dt, device=self.device), self.fill)
            for g in self.guards(i):
                b = (_bits(g) != _bits(want)).any()
                bad = b if bad is None else bad | b
        return bad is None or not bool(bad)


class Placed(dict):
    """Tensors that lie in an Arena already (Arena.place_all): .arena is that arena."""
    arena = None


def _bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def same_bits(a, b, names=("the first", "the second")):
    """None where a and b have the same bit patterns, else the count, the first (row, column) and both values there."""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    bad = _bits(a) != _bits(b)
    n = int(bad.sum())
    if n == 0:
        return None
    cols = a.shape[-1] if a.dim() else 1
    i = int(bad.reshape(-1).nonzero()[0])
    x, y = a.reshape(-1)[i:i + 1], b.reshape(-1)[i:i + 1]
    return (f"{n} of {bad.numel()} elements differ, the first at (row {i // cols}, column {i % cols}): {names[0]} has {float(x)!r} "
            f"({int(_bits(x)) & (1 << 8 * x.element_size()) - 1:#x}), {names[1]} {float(y)!r} ({int(_bits(y)) & (1 << 8 * y.element_size()) - 1:#x})")
