"""Score curves on the GPU (`pytest -m gpu`), through the C ABI of include/ovmr_hip_curves.h: after every call the state is BIT-EQUAL to
the brute-force reference of curves_cases.py -- the edge table of the slot function spread over rows and columns, every row and class
count at which the kernel's indexing changes, unaligned and padded rows, labels that belong to no class, a pre-filled state, any cut
and order of the rows, guarded buffers under four fills, a captured graph.  Nothing here carries a tolerance."""
import ctypes

import pytest
import torch

import curves_cases as K
import poison

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import runtime
    return runtime.load_library()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(lib, out, ld, y, B, C, lo, hi, bins, state):
    return lib.ovmr_eval_curves(_p(out), int(out.dtype == torch.float32), ld, _p(y), B, C, lo, hi, bins, _p(state), _s())


def _run(lib, out, y, lo, hi, bins, before, gap=0, fill="nan16", spans=None):
    """The rows of `out` ([B, C] on the host) offered span by span (default: whole), each batch a guarded buffer of its own with rows
    C + gap apart, ONE ELEMENT off the allocation's alignment and `fill` in the gaps; the state starts as `before` inside its own guards.
    -> the state on the host, int32 [C, 2, bins + 3]; every guard is checked."""
    B, C = out.shape
    ld = C + gap
    arena = poison.Arena(fill, DEV, guard=256)
    state = arena.place(before.int())
    for a, b in spans if spans is not None else [(0, B)]:
        n = b - a
        flat = arena.take(1 + max(n, 1) * ld, poison.kind_of(out))[1:]
        rows = flat[:n * ld].view(n, ld)
        rows[:, :C] = out[a:b].to(DEV)
        lab = arena.place(y[a:b].contiguous()) if n else arena.take(1, "i64")
        # (the address is flat's: an empty view answers data_ptr() with 0, and B == 0 excuses no NULL)
        assert lib.ovmr_eval_curves(_p(flat), int(out.dtype == torch.float32), ld, _p(lab), n, C, lo, hi, bins, _p(state), _s()) == 0, (a, b)
    torch.cuda.synchronize()
    assert arena.intact(), "a guard region was written"
    return state.cpu()


def _check(lib, B, C, lo, hi, bins, fp16, kind="random", gap=0, fill="nan16", seed=0, softmax=False):
    out = K.scores(B, C, lo, hi, bins, fp16, seed, "softmax" if softmax else "uniform")
    y = K.labels(B, C, kind, seed)
    before = K.random_state(C, bins, seed)
    got = _run(lib, out, y, lo, hi, bins, before, gap, fill)
    msg = K.mismatch(got, K.expected(out, y, lo, hi, bins, before))
    assert msg is None, (B, C, lo, hi, bins, fp16, kind, gap, msg)


ROWS = [1, 63, 64, 65, 130]                                     # a chunk of 64 rows less and more, two chunks and a part
CLASSES = [1, 3, 15, 16, 17, 31, 32, 33]                        # a tile of 16 classes less and more, twice; odd C: unaligned fp16 rows


@pytest.mark.parametrize("fp16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("B", ROWS)
def test_every_row_and_class_count(lib, B, fp16):
    """Each (B, C) with another of the bins, ranges, label kinds and row pitches, so that all of them meet all sizes over the table."""
    for i, C in enumerate(CLASSES):
        n = i + ROWS.index(B) + int(fp16)
        lo, hi = K.RANGES[n % 3]
        _check(lib, B, C, lo, hi, K.BINS[n % 4], fp16, ("random", "hot", "bad")[n % 3], gap=(0, 3)[(n // 2) % 2], seed=n, softmax=n % 5 == 0)


@pytest.mark.parametrize("lo,hi,bins", [(lo, hi, b) for lo, hi in K.RANGES for b in K.BINS] + K.CLAMP_CASES)
def test_edge_table_over_rows_and_columns(lib, lo, hi, bins):
    """130 x 33 scores hold the whole edge table (checked), fp32 and fp16; an odd C with ld == C leaves every second fp16 row unaligned."""
    for fp16 in (False, True):
        assert len(K.edge_table(lo, hi, bins, fp16)) <= 130 * 33
        _check(lib, 130, 33, lo, hi, bins, fp16, "bad", gap=0, seed=bins)


@pytest.mark.parametrize("fill", sorted(poison.FILLS))
def test_guards_and_gaps_under_every_fill(lib, fill):
    for fp16, C, gap in ((True, 17, 0), (True, 33, 5), (False, 17, 3), (False, 1, 0)):
        _check(lib, 65, C, 0.0, 1.0, 7, fp16, "bad", gap=gap, fill=fill, seed=1)


def test_more_rows_than_one_sweep(lib):
    """gridDim.y stops at MAX_ROW_BLOCKS chunks: with more rows a workgroup takes several.  Both sides of that, and a ragged end."""
    full = K.CHUNK * K.MAX_ROW_BLOCKS
    for B, C in ((full, 3), (full + 1, 1), (2 * full + 65, 3)):
        _check(lib, B, C, 0.0, 1.0, 7, True, "random", seed=B, softmax=True)


def test_hot_cell_and_softmax_rows(lib):
    """Every row one label and softmax rows: nearly all negatives of a class in ONE cell, all positives in one class."""
    for bins in (1, 256):
        _check(lib, 130, 33, 0.0, 1.0, bins, False, "hot", seed=4, softmax=True)
    out = torch.zeros((130, 17), dtype=torch.float16)
    y = torch.full((130,), 5, dtype=torch.int64)
    got = _run(lib, out, y, 0.0, 1.0, 16, torch.zeros((17, 2, 19), dtype=torch.int64))
    want = torch.zeros((17, 2, 19), dtype=torch.int32)
    want[:, 0, 1] = 130
    want[5, 0, 1], want[5, 1, 1] = 0, 130
    assert torch.equal(got, want)


def test_labels_outside_the_classes_are_offered_to_no_class(lib):
    C, bins = 17, 16
    out = K.scores(8, C, 0.0, 1.0, bins, False, seed=2)
    y = torch.tensor([-1, C, 2 ** 40, 3, -2 ** 63, 2 ** 63 - 1, 2 ** 32 + 3, 0])
    got = _run(lib, out, y, 0.0, 1.0, bins, torch.zeros((C, 2, bins + 3), dtype=torch.int64))
    assert K.mismatch(got, K.expected(out, y, 0.0, 1.0, bins)) is None
    assert int(got.sum()) == 2 * C and int(got[:, 1].sum()) == 2 and int(got[3, 1].sum()) == 1 and int(got[0, 1].sum()) == 1


def test_every_cut_and_order_gives_the_same_bytes(lib):
    B, C, lo, hi, bins = 130, 33, 0.1, 0.7, 256
    out, y = K.scores(B, C, lo, hi, bins, True, seed=6), K.labels(B, C, "bad", seed=6)
    before = K.random_state(C, bins, seed=6)
    whole = _run(lib, out, y, lo, hi, bins, before, gap=3)
    assert K.mismatch(whole, K.expected(out, y, lo, hi, bins, before)) is None
    for step in (1, 7, 64):
        spans = [(a, min(a + step, B)) for a in range(0, B, step)]
        for order in (spans, spans[::-1]):
            got = _run(lib, out, y, lo, hi, bins, before, gap=3, spans=order)
            assert torch.equal(got, whole), (step, order is spans)


def test_empty_batch_leaves_the_state_alone(lib):
    out, y = K.scores(5, 17, 0.0, 1.0, 7), K.labels(5, 17)
    before = K.random_state(17, 7, seed=8)
    got = _run(lib, out, y, 0.0, 1.0, 7, before, spans=[(0, 0), (5, 5)])
    assert torch.equal(got.long(), before)
    state = torch.zeros((17, 2, 10), dtype=torch.int32, device=DEV)
    lab = torch.zeros(4, dtype=torch.int64, device=DEV)
    x = torch.zeros((4, 17), device=DEV)
    for bad in (dict(ld=16), dict(bins=0), dict(bins=4097), dict(lo=1.0), dict(hi=float("inf"))):
        a = dict(ld=17, lo=0.0, hi=1.0, bins=7)
        a.update(bad)
        shaped = state if a["bins"] == 7 else torch.zeros((17, 2, 4100), dtype=torch.int32, device=DEV)
        assert lib.ovmr_eval_curves(_p(x), 1, a["ld"], _p(lab), 4, 17, a["lo"], a["hi"], a["bins"], _p(shaped), _s()) == -1, bad
    torch.cuda.synchronize()
    assert not bool(state.any()), "an argument error writes nothing"


def test_graph_replay(lib):
    """The call captured on a single stream and replayed twice equals two eager calls."""
    B, C, lo, hi, bins = 65, 33, 0.0, 1.0, 256
    out, y = K.scores(B, C, lo, hi, bins, False, seed=9, kind="softmax"), K.labels(B, C, seed=9)
    once = K.expected(out, y, lo, hi, bins)
    dev, lab = out.to(DEV), y.to(DEV)
    state = torch.zeros((C, 2, bins + 3), dtype=torch.int32, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert _call(lib, dev, C, lab, B, C, lo, hi, bins, state) == 0
    torch.cuda.synchronize()
    assert not bool(state.any())                                        # (capture itself runs nothing)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    eager = torch.zeros_like(state)
    for _ in range(2):
        assert _call(lib, dev, C, lab, B, C, lo, hi, bins, eager) == 0
    torch.cuda.synchronize()
    assert torch.equal(state, eager) and K.mismatch(state.cpu(), 2 * once) is None


def test_wrapper_on_a_row_view_of_a_wider_matrix(lib):
    from ovmr_amd import runtime
    B, C, lo, hi, bins = 130, 33, -100.0, 100.0, 1024
    for fp16 in (False, True):
        out, y = K.scores(B, C, lo, hi, bins, fp16, seed=10), K.labels(B, C, "bad", seed=10)
        wide = torch.full((B, C + 8), float("nan"), dtype=out.dtype, device=DEV)
        wide[:, 3:3 + C] = out.to(DEV)
        state = torch.zeros((C, 2, bins + 3), dtype=torch.int32, device=DEV)
        runtime.eval_curves(wide[:100, 3:3 + C], y[:100].to(DEV), lo, hi, bins, state)
        runtime.eval_curves(wide[100:, 3:3 + C], y[100:].to(DEV), lo, hi, bins, state)
        runtime.eval_curves(wide[:0, 3:3 + C], y[:0].to(DEV), lo, hi, bins, state)
        assert K.mismatch(state.cpu(), K.expected(out, y, lo, hi, bins)) is None, fp16
