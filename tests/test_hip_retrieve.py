"""Search by class on the GPU (`pytest -m gpu`), through the C ABI of include/ovmr_hip_retrieve.h: every pool of retrieve_cases.py fed in
several cuts and in reversed batch order must leave a BYTE-EQUAL state and the expected finish; floors, merges, image indices around 2^31
and at the end of the range, guarded buffers.  Nothing here carries a tolerance: indices and state bytes bit for bit, values as numbers
with NaN == NaN."""
import ctypes
import math

import pytest
import torch

import retrieve_cases as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                    # elements of guard before and after a buffer


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import runtime
    return runtime.load_library()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """n elements with a guard region of a known pattern on either side; .t is the inner view."""

    PATTERN = {torch.int64: 0x5A5A5A5A5A5A5A5A, torch.float32: -12345.0}

    def __init__(self, n, dtype, fill):
        self.n, self.pat = n, self.PATTERN[dtype]
        self.all = torch.full((n + 2 * GUARD,), self.pat, dtype=dtype, device=DEV)
        self.t = self.all[GUARD:GUARD + n]
        self.t.fill_(fill)

    def intact(self):
        return bool((self.all[:GUARD] == self.pat).all()) and bool((self.all[GUARD + self.n:] == self.pat).all())


def _spans(cuts, reverse=False):
    spans, a = [], 0
    for n in cuts:
        spans.append((a, a + n))
        a += n
    return spans[::-1] if reverse else spans


def _feed(lib, state, s, m, spans, base=0, gap=0, floor=None):
    """ovmr_retrieve_update for the rows [a, b) of pool s, each batch a slice of a larger NaN-poisoned buffer: rows C + gap apart, one
    element off the allocation's alignment, NaNs in the gap and after the last row."""
    C = s.shape[1]
    ld = C + gap
    keep = []
    for a, b in spans:
        big = torch.full((1 + (b - a) * ld + C + 16,), math.nan, dtype=s.dtype, device=DEV)
        out = big[1:1 + (b - a) * ld].view(b - a, ld)
        out[:, :C] = s[a:b].to(DEV)
        f = None if floor is None else floor[a:b].to(DEV).contiguous()
        rc = lib.ovmr_retrieve_update(_p(out), int(s.dtype == torch.float32), ld, b - a, C, m, base + a, None if f is None else _p(f),
                                      _p(state.t), _stream())
        assert rc == 0, (rc, a, b)
        keep += [big, f]
    torch.cuda.synchronize()


def _new_state(lib, C, m):
    st = Guarded(C * m, torch.int64, 0x7777)                 # (reset must empty it)
    assert lib.ovmr_retrieve_reset(_p(st.t), C, m, _stream()) == 0
    return st


def _finish(lib, st, C, m):
    v, i = Guarded(C * m, torch.float32, 777.0), Guarded(C * m, torch.int64, 0x1234567)      # every element must be overwritten
    assert lib.ovmr_retrieve_finish(_p(st.t), C, m, _p(v.t), _p(i.t), _stream()) == 0
    torch.cuda.synchronize()
    assert v.intact() and i.intact() and st.intact(), "a guard region was written"
    return v.t.view(C, m).cpu(), i.t.view(C, m).cpu()


def _search(lib, s, m, cuts, reverse=False, **kw):
    C = s.shape[1]
    st = _new_state(lib, C, m)
    _feed(lib, st, s, m, _spans(cuts, reverse), **kw)
    return st.t.cpu().clone(), _finish(lib, st, C, m)


# (N, C, m, dtype, gap): the smallest sizes at which each index can go wrong -- one class, a tile of 4 / 16 classes and 64 classes
# less and more, an odd C (unaligned fp16 rows), a chunk of 64 rows less and more, pools shorter than m
SHAPES = [(300, 130, 5, torch.float16, 0), (300, 65, 32, torch.float16, 3), (300, 1001, 2, torch.float16, 0), (300, 64, 31, torch.float32, 3),
          (300, 1001, 5, torch.float32, 3), (65, 63, 1, torch.float32, 0), (65, 130, 31, torch.float16, 3), (64, 1, 5, torch.float16, 0),
          (64, 65, 32, torch.float32, 0), (63, 65, 32, torch.float16, 3), (5, 130, 32, torch.float32, 0), (5, 63, 5, torch.float16, 3),
          (1, 64, 5, torch.float16, 3), (1, 1, 1, torch.float32, 0),
          # up to R.NARROW_MAX_C = 2048 classes a workgroup owns 4 classes (one per wave), beyond it 16: both sides of the threshold, and the
          # 16-class tiles with an odd C, a partial last tile, padded rows, a pool shorter than m
          (300, 2048, 31, torch.float16, 3), (65, 2048, 5, torch.float32, 0), (300, 2049, 5, torch.float16, 0), (300, 2113, 32, torch.float32, 3),
          (65, 2049, 2, torch.float16, 3), (64, 2062, 32, torch.float16, 0), (5, 2050, 32, torch.float32, 3), (1, 2049, 1, torch.float16, 0)]


@pytest.mark.parametrize("N,C,m,dtype,gap", SHAPES, ids=[f"N{n}-C{c}-m{m}-{'f16' if d == torch.float16 else 'f32'}-gap{g}" for n, c, m, d, g in SHAPES])
def test_every_cut_gives_the_same_state_and_the_expected_lists(lib, N, C, m, dtype, gap):
    s = R.planted_pool(N, C, dtype)
    want = R.expected(s, m)
    first = None
    for cuts in R.CUTS[N]:
        for reverse in (False, True) if len(cuts) > 1 else (False,):
            state, got = _search(lib, s, m, cuts, reverse, gap=gap)
            assert R.mismatch(got, want) is None, (cuts, reverse, R.mismatch(got, want))
            first = state if first is None else first
            assert torch.equal(state, first), f"cuts {cuts}, reversed {reverse}: the state differs from that of {R.CUTS[N][0]}"
    if N >= 281 and m == 2:
        assert got[1][0].tolist() == [3, 90], "images 3, 90 and 280 share the best value: the tie decides membership"


def test_all_zero_matrix_answers_the_first_images(lib):
    s = torch.zeros((300, 65), dtype=torch.float16)
    s[2::5] = -0.0
    _, (v, i) = _search(lib, s, 32, (65, 235), True)
    assert torch.equal(i, torch.arange(32).expand(65, 32)) and bool((v == 0).all()) and not bool(torch.signbit(v).any()), "-0 is reported as +0"


@pytest.mark.parametrize("N,C,m", [(65, 17, 31), (300, 130, 5), (65, 2049, 5)])
def test_floor(lib, N, C, m):
    s = R.planted_pool(N, C)
    floor = R.floor_table(s)
    want = R.expected(s, m, floor)
    assert R.mismatch(want, R.expected(s, m)) is not None
    first = None
    for cuts in R.CUTS[N]:
        state, got = _search(lib, s, m, cuts, floor=floor, gap=3)
        assert R.mismatch(got, want) is None, (cuts, R.mismatch(got, want))
        first = state if first is None else first
        assert torch.equal(state, first)
    everything = torch.full((N,), -math.inf)
    assert R.mismatch(_search(lib, s, m, (N,), floor=everything)[1], R.expected(s, m)) is None, "a floor of -inf admits everything"


def test_merge(lib):
    N, C, m, cut = 300, 130, 5, 100
    s = R.planted_pool(N, C)
    single, want = _search(lib, s, m, (N,))
    assert R.mismatch(want, R.expected(s, m)) is None
    for order in ("AB", "BA"):
        a, b = _new_state(lib, C, m), _new_state(lib, C, m)
        _feed(lib, a, s, m, [(0, cut)])
        _feed(lib, b, s, m, [(cut, N)])
        dst, src = (a, b) if order == "AB" else (b, a)
        before = src.t.cpu().clone()
        assert lib.ovmr_retrieve_merge(_p(dst.t), _p(src.t), C, m, _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(dst.t.cpu(), single), order
        assert torch.equal(src.t.cpu(), before) and dst.intact() and src.intact()
        empty = _new_state(lib, C, m)
        assert lib.ovmr_retrieve_merge(_p(dst.t), _p(empty.t), C, m, _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(dst.t.cpu(), single), "merging an empty state changes nothing"
        assert lib.ovmr_retrieve_merge(_p(empty.t), _p(dst.t), C, m, _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(empty.t.cpu(), single), "merging into an empty state copies the lists"


@pytest.mark.parametrize("base", [2 ** 31 - 3, 2 ** 32 - 1 - 8])
def test_large_bases(lib, base):
    s = R.planted_pool(8, 8)
    for m in (5, 32):
        want = R.expected(s, m, base=base)
        assert want[1][1, :5].tolist() == [base + j for j in range(5)], "the all-zero column: ties to the lower index, across 2^31"
        for cuts in ((8,), (3, 5)):
            for reverse in (False, True):
                got = _search(lib, s, m, cuts, reverse, base=base)[1]
                assert R.mismatch(got, want) is None, (cuts, reverse, R.mismatch(got, want))
        assert int(want[1].max()) == base + 7 and got[1].dtype == torch.int64


def test_empty_batch_leaves_the_state_alone(lib):
    s = R.planted_pool(65, 17)
    st = _new_state(lib, 17, 5)
    _feed(lib, st, s, 5, [(0, 65)])
    before = st.all.cpu().clone()
    out = torch.full((17,), math.nan, dtype=torch.float16, device=DEV)
    assert lib.ovmr_retrieve_update(_p(out), 0, 17, 0, 17, 5, 65, None, _p(st.t), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(st.all.cpu(), before)


def test_column_top_m_wrapper(lib):
    """runtime.ColumnTopM on row views of a wider matrix, with a floor, merged through its state tensor."""
    from ovmr_amd import runtime
    s = R.planted_pool(300, 130)
    floor = R.floor_table(s)
    wide = torch.full((300, 140), math.nan, dtype=torch.float16, device=DEV)
    wide[:, 3:133] = s.to(DEV)
    a, b = runtime.ColumnTopM(130, 5, DEV), runtime.ColumnTopM(130, 5, DEV)
    a.update(wide[:100, 3:133], 0, floor[:100].to(DEV))
    b.update(wide[100:, 3:133], 100, floor[100:].to(DEV)).update(wide[:0, 3:133], 300)
    a.merge(b.state.clone())
    assert R.mismatch(tuple(t.cpu() for t in a.finish()), R.expected(s, 5, floor)) is None
    assert R.mismatch(tuple(t.cpu() for t in b.reset().finish()), R.expected(s[:0], 5)) is None
