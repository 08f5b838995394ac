"""Exact ranking counts on the GPU (`pytest -m gpu`), through the C ABI of include/ovmr_hip_ranks.h: after every call the int32 state is
BIT-EQUAL to the brute-force reference of ranks_cases.py -- every row and class count at which the kernel's indexing changes, unaligned and
padded rows, every edge count at which the search changes (none, one, a power of two less and more, the LDS staging threshold less and
more), a class beyond max_edges, one hot cell, softmax rows, the values the order can go wrong at, labels that belong to no class, more
rows than one sweep, any cut and order of the rows, guarded buffers under four fills with a garbage estart, a captured graph.  Nothing
here carries a tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import poison
import ranks_cases as K

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


def _run(lib, out, y, edges, estart, max_edges, before, gap=0, fill="nan16", spans=None):
    """The rows of `out` ([B, C] on the host) offered span by span (default: whole), each batch a guarded buffer of its own with rows
    C + gap apart, ONE ELEMENT off the allocation's alignment and `fill` in the gaps; edges, estart and the state (which starts as
    `before`) lie inside guards of their own.  -> the state on the host, int32 [2, 2E + C]; every guard is checked."""
    B, C = out.shape
    E = len(edges)
    ld = C + gap
    arena = poison.Arena(fill, DEV, guard=256)
    state = arena.place(before.int())
    ed = arena.take(max(E, 1), "f32")[:E]
    ed.copy_(torch.from_numpy(np.asarray(edges, dtype=np.float32)))
    es = arena.place(torch.from_numpy(np.asarray(estart, dtype=np.int32)))
    for a, b in spans if spans is not None else [(0, B)]:
        n = b - a
        flat = arena.take(1 + max(n, 1) * ld, poison.kind_of(out))[1:]
        rows = flat[:n * ld].view(n, ld)
        rows[:, :C] = out[a:b].to(DEV)
        lab = arena.place(y[a:b].contiguous()) if n else arena.take(1, "i64")
        rc = lib.ovmr_eval_ranks(_p(flat), int(out.dtype == torch.float32), ld, _p(lab), n, C, _p(ed) if E else None, _p(es), E, max_edges,
                                 _p(state), _s())
        assert rc == 0, (a, b, rc)
    torch.cuda.synchronize()
    assert arena.intact(), "a guard region was written"
    return state.cpu().view(2, 2 * E + C)


def _check(lib, B, counts, fp16, kind="mixed", label_kind="random", gap=0, fill="nan16", seed=0, special=False, max_edges=None):
    C = len(counts)
    edges, estart = K.make_edges(counts, seed, special, fp16)
    out = K.scores(B, C, edges, estart, kind, fp16, seed)
    y = K.labels(B, C, label_kind, seed)
    me = max(counts) if max_edges is None else max_edges
    before = K.random_state(C, len(edges), seed)
    got = _run(lib, out, y, edges, estart, me, before, gap, fill)
    msg = K.mismatch(got, K.expected(out, y, edges, estart, me, before))
    assert msg is None, (B, counts, fp16, kind, label_kind, gap, msg)


ROWS = [1, 63, 64, 65, 257]
CLASSES = [1, 15, 16, 17, 33]
EDGE_COUNTS = [0, 1, 2, 63, 64, 65, K.STAGE - 1, K.STAGE, K.STAGE + 1]


def _counts(C, n):
    """C edge counts walking EDGE_COUNTS from position n: the small ones often, the large ones once per 9 classes."""
    return [EDGE_COUNTS[(n + 4 * i) % 9] if i % 3 == 0 else EDGE_COUNTS[(n + i) % 3] for i in range(C)]


@pytest.mark.parametrize("fp16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("B", ROWS)
def test_every_row_and_class_count(lib, B, fp16):
    """Each (B, C) with another of the edge counts, score kinds, label kinds and row pitches, so that all of them meet all sizes over the
    table; an odd C with ld == C leaves every second fp16 row unaligned."""
    for i, C in enumerate(CLASSES):
        n = i + ROWS.index(B) + int(fp16)
        _check(lib, B, _counts(C, n), fp16, ("mixed", "special", "softmax")[n % 3], ("random", "hot", "bad")[n % 3], gap=(0, 3)[(n // 2) % 2],
               seed=n, special=n % 2 == 0)


@pytest.mark.parametrize("n", EDGE_COUNTS)
def test_every_edge_count(lib, n):
    """Every class of a tile with n edges, fp32 and fp16, special values among scores and edges: the staging threshold on both sides."""
    for fp16 in (False, True):
        _check(lib, 130, [n] * 17, fp16, "special", "bad", seed=n, special=True)


def test_class_beyond_max_edges(lib):
    """max_edges below a class's count: the class is searched against its first max_edges edges, and its base stays 2 estart[c] + c."""
    for me in (0, 1, 5, 64):
        _check(lib, 130, [9, 70, 0, 3, 300], False, "mixed", "random", seed=me, max_edges=me)


def test_hot_cell_and_softmax_rows(lib):
    """All scores equal (one hot cell per class and plane) and softmax rows under one label: nearly every negative in the last cell."""
    _check(lib, 130, [5] * 33, False, "equal", "hot", seed=1)
    _check(lib, 130, [5] * 33, True, "equal", "random", seed=2)
    _check(lib, 257, _counts(33, 0), False, "softmax", "hot", seed=3)
    C, B = 17, 130
    edges, estart = np.array([0.5, 0.25, 0.125], dtype=np.float32), np.array([0] * 6 + [3] * 12, dtype=np.int32)      # class 5 alone has edges
    got = _run(lib, torch.full((B, C), 0.25, dtype=torch.float16), torch.full((B,), 5, dtype=torch.int64), edges, estart, 3,
               torch.zeros((2, 6 + C), dtype=torch.int64))
    want = torch.zeros((2, 6 + C), dtype=torch.int32)
    for c in range(C):
        want[0, 2 * int(estart[c]) + c] = B
    want[0, 5], want[1, 5 + 3] = 0, B                                # class 5: every row its own, tied with edge 1
    assert torch.equal(got, want)


def test_labels_outside_the_classes_are_offered_to_no_class(lib):
    C = 17
    edges, estart = K.make_edges([3] * C, seed=2)
    out = K.scores(8, C, edges, estart, "mixed", seed=2)
    y = torch.tensor([-1, C, 2 ** 40, 3, -2 ** 63, 2 ** 63 - 1, 2 ** 32 + 3, 0])
    got = _run(lib, out, y, edges, estart, 3, torch.zeros((2, 2 * len(edges) + C), dtype=torch.int64))
    assert K.mismatch(got, K.expected(out, y, edges, estart, 3)) is None
    assert int(got.sum()) == 2 * C and int(got[1].sum()) == 2


def test_more_rows_than_one_sweep(lib):
    """gridDim.y stops at MAX_ROW_BLOCKS chunks: with 16 385 rows a workgroup takes a second chunk."""
    B = K.CHUNK * K.MAX_ROW_BLOCKS + 1
    _check(lib, B, [2, 65], True, "softmax", "random", seed=B)


def test_every_cut_and_order_gives_the_same_bytes(lib):
    B, counts = 130, _counts(33, 5)
    C = len(counts)
    edges, estart = K.make_edges(counts, 6, True, True)
    out, y = K.scores(B, C, edges, estart, "special", True, seed=6), K.labels(B, C, "bad", seed=6)
    before = K.random_state(C, len(edges), seed=6)
    whole = _run(lib, out, y, edges, estart, max(counts), before, gap=3)
    assert K.mismatch(whole, K.expected(out, y, edges, estart, max(counts), before)) is None
    for step in (1, 7, 64):
        spans = [(a, min(a + step, B)) for a in range(0, B, step)]
        for order in (spans, spans[::-1]):
            got = _run(lib, out, y, edges, estart, max(counts), before, gap=3, spans=order)
            assert torch.equal(got, whole), (step, order is spans)


def test_empty_batch_and_argument_errors_leave_the_state_alone(lib):
    counts = [3] * 17
    edges, estart = K.make_edges(counts, 8)
    out, y = K.scores(5, 17, edges, estart, seed=8), K.labels(5, 17)
    before = K.random_state(17, len(edges), seed=8)
    got = _run(lib, out, y, edges, estart, 3, before, spans=[(0, 0), (5, 5)])
    assert torch.equal(got.long(), before)
    E = len(edges)
    state = torch.zeros((2, 2 * E + 17), dtype=torch.int32, device=DEV)
    lab, x = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros((4, 17), device=DEV)
    ed, es = torch.from_numpy(edges).to(DEV), torch.from_numpy(estart).to(DEV)
    for bad in (dict(ld=16), dict(E=-1), dict(me=-1), dict(me=E + 1), dict(ed=None), dict(es=None)):
        a = dict(ld=17, E=E, me=3, ed=_p(ed), es=_p(es))
        a.update(bad)
        assert lib.ovmr_eval_ranks(_p(x), 1, a["ld"], _p(lab), 4, 17, a["ed"], a["es"], a["E"], a["me"], _p(state), _s()) == -1, bad
    torch.cuda.synchronize()
    assert not bool(state.any()), "an argument error writes nothing"


@pytest.mark.parametrize("fill", sorted(poison.FILLS))
def test_guards_under_every_fill_and_a_garbage_estart(lib, fill):
    """The four poison fills around state, edges, estart and outputs; then an estart of garbage (negative, beyond E, decreasing, int32
    extremes): whatever is counted, it is counted INSIDE the state -- every offered (row, class) exactly once -- and no guard is touched."""
    for fp16, C, gap in ((True, 17, 0), (True, 33, 5), (False, 17, 3), (False, 1, 0)):
        _check(lib, 65, _counts(C, 1), fp16, "special", "bad", gap=gap, fill=fill, seed=1, special=True)
    C, B = 19, 65
    edges, _ = K.make_edges([40] * C, seed=3)
    E = len(edges)
    garbage = np.array([5, -7, E + 100, 3, 2 ** 31 - 1, -2 ** 31, E, E - 1, 0, 900, 10, 10, 700, 2, E + 1, -1, 64, 63, 1000, 0], dtype=np.int32)
    out, y = K.scores(B, C, edges, np.arange(0, E + 1, 40), "mixed", seed=4), K.labels(B, C, "bad", seed=4)
    offered = int(((y >= 0) & (y < C)).sum())
    for me in (E, 300, 7):
        got = _run(lib, out, y, edges, garbage, me, torch.zeros((2, 2 * E + C), dtype=torch.int64), fill=fill)
        assert int(got.sum()) == offered * C and int(got.min()) >= 0 and int(got[1].sum()) == offered
        # (a clamped range may straddle two classes' edges and not descend: the search still ends somewhere, where the model's does)
        want, outside = K.model(out, y, edges, garbage, me, torch.zeros((2, 2 * E + C), dtype=torch.int64))
        assert outside == 0 and K.mismatch(got, want) is None, me


def test_graph_replay(lib):
    """The call captured on a single stream and replayed twice equals two eager calls."""
    B, counts = 65, _counts(33, 2)
    C = len(counts)
    edges, estart = K.make_edges(counts, 9)
    out, y = K.scores(B, C, edges, estart, "softmax", seed=9), K.labels(B, C, seed=9)
    once = K.expected(out, y, edges, estart)
    dev, lab, ed, es = out.to(DEV), y.to(DEV), torch.from_numpy(edges).to(DEV), torch.from_numpy(estart).to(DEV)
    E = len(edges)
    call = lambda st: lib.ovmr_eval_ranks(_p(dev), 1, C, _p(lab), B, C, _p(ed), _p(es), E, max(counts), _p(st), _s())      # noqa: E731
    state = torch.zeros((2, 2 * E + C), dtype=torch.int32, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert call(state) == 0
    torch.cuda.synchronize()
    assert not bool(state.any())                                        # (capture itself runs nothing)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    eager = torch.zeros_like(state)
    for _ in range(2):
        assert call(eager) == 0
    torch.cuda.synchronize()
    assert torch.equal(state, eager) and K.mismatch(state.cpu(), 2 * once) is None


def test_wrapper_on_a_row_view_of_a_wider_matrix(lib):
    from ovmr_amd import runtime
    B, counts = 130, _counts(33, 7)
    C = len(counts)
    for fp16 in (False, True):
        edges, estart = K.make_edges(counts, 10, True, fp16)
        out, y = K.scores(B, C, edges, estart, "special", fp16, seed=10), K.labels(B, C, "bad", seed=10)
        wide = torch.full((B, C + 8), float("nan"), dtype=out.dtype, device=DEV)
        wide[:, 3:3 + C] = out.to(DEV)
        ed, es = torch.from_numpy(edges).to(DEV), torch.from_numpy(estart).to(DEV)
        state = torch.zeros((2, 2 * len(edges) + C), dtype=torch.int32, device=DEV)
        for a, b in ((0, 100), (100, B), (0, 0)):
            runtime.eval_ranks(wide[a:b, 3:3 + C], y[a:b].to(DEV), ed, es, state, max(counts))
        assert K.mismatch(state.cpu(), K.expected(out, y, edges, estart)) is None, fp16
    none = torch.zeros(0, dtype=torch.float32, device=DEV)                # a pass without a positive: one cell per class
    state = torch.zeros((2, C), dtype=torch.int32, device=DEV)
    runtime.eval_ranks(wide[:, 3:3 + C], y.to(DEV), none, torch.zeros(C + 1, dtype=torch.int32, device=DEV), state, 0)
    assert K.mismatch(state.cpu(), K.expected(out, y, np.zeros(0, dtype=np.float32), np.zeros(C + 1, dtype=np.int32))) is None
