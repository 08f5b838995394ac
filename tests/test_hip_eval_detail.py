"""ovmr_eval_detail (csrc/eval_detail.hip) at the C ABI, through ctypes, in fp16 and fp32.  The expectation comes from the CPU: the k columns
of a row are those of the stable descending sort, torch.sort(x.float(), dim=1, descending=True, stable=True)[1][:, :k] (larger value first,
equal values in increasing column order, NaN above +inf, -0 == +0), the histograms are built with np.add.at.  Everything is an integer and
compared exactly.  Run with -m gpu on an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
SPECIAL_ROW = [1, NAN, 3, 3, -0.0, 0.0, INF, NAN, -INF, 3]
DTYPES = [torch.float16, torch.float32]
# (B, C, k, ld, with cmat): the shapes of tests/test_hip_topk.py, a batch of several workgroups with a ragged last one, and C = 4099 with
# its 67 MB confusion matrix; at 21 841 classes cmat is NULL (1.9 GB: not tested)
SHAPES = [(1, 1, 1, None, True), (3, 7, 7, None, True), (5, 63, 5, None, True), (5, 64, 5, None, True), (5, 65, 5, None, True),
          (4, 257, 8, 263, True), (4, 264, 32, 264, True), (257, 101, 1, None, True), (6, 1000, 5, None, True), (8, 4099, 5, None, True),
          (2, 21841, 10, None, False)]
POISON = -7


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import runtime
    return runtime.load_library()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _code(dtype):
    return 1 if dtype == torch.float32 else 0


def _strided(x, ld):
    """x [B, C] on the GPU as a row view of a [B, ld] buffer whose padding holds NaN (never to be read)."""
    B, C = x.shape
    if ld is None or ld == C:
        return x.cuda().contiguous(), C
    wide = torch.full((B, ld), NAN, dtype=x.dtype)
    wide[:, :C] = x
    return wide.cuda()[:, :C], ld


def _random(B, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, C), generator=g).half().to(dtype)           # fp16-rounded normals: ties occur naturally


def _order(x):
    return torch.sort(x.float(), dim=1, descending=True, stable=True)[1]


def _want(x, labels, k, cmat=True):
    """(counts [3C + 1], hits, class_hits [C], cmat [C, C] or None) as int64 NumPy arrays."""
    B, C = x.shape
    top = _order(x)[:, :k].numpy()
    lab = np.asarray(labels, dtype=np.int64)
    ok = (lab >= 0) & (lab < C)
    pred, g = top[ok, 0], lab[ok]
    counts = np.zeros(3 * C + 1, dtype=np.int64)
    np.add.at(counts, pred[pred == g], 1)
    np.add.at(counts, C + pred, 1)
    np.add.at(counts, 2 * C + g, 1)
    counts[3 * C] = int((~ok).sum())
    hit = (top[ok] == g[:, None]).any(axis=1)
    class_hits = np.zeros(C, dtype=np.int64)
    np.add.at(class_hits, g[hit], 1)
    cm = None
    if cmat:
        cm = np.zeros((C, C), dtype=np.int64)
        np.add.at(cm, (g, pred), 1)
    return counts, int(hit.sum()), class_hits, cm


class Buffers:
    def __init__(self, C, hits=True, class_hits=True, cmat=True, fill=0):
        new = lambda *shape: torch.full(shape, fill, dtype=torch.int32, device="cuda")     # noqa: E731
        self.counts = new(3 * C + 1)
        self.hits = new(1) if hits else None
        self.class_hits = new(C) if class_hits else None
        self.cmat = new(C, C) if cmat else None

    def host(self):
        f = lambda t: None if t is None else t.cpu().long().numpy()     # noqa: E731
        return f(self.counts), None if self.hits is None else int(self.hits.cpu()), f(self.class_hits), f(self.cmat)


def _call(lib, x, labels, k, buf, ld=None):
    dev, ld = _strided(x, ld)
    B, C = x.shape
    lab = torch.as_tensor(labels, dtype=torch.int64).cuda()
    rc = lib.ovmr_eval_detail(_p(dev), _code(x.dtype), ld, _p(lab), B, C, k, _p(buf.counts), _p(buf.hits), _p(buf.class_hits), _p(buf.cmat), _s())
    torch.cuda.synchronize()
    return rc


def _assert_equal(got, want, times=1):
    counts, hits, class_hits, cm = got
    w_counts, w_hits, w_class_hits, w_cm = want
    assert np.array_equal(counts, times * w_counts)
    if hits is not None:
        assert hits == times * w_hits
    if class_hits is not None:
        assert np.array_equal(class_hits, times * w_class_hits)
    if cm is not None:
        assert np.array_equal(cm, times * w_cm)


def _identities(got, C, k):
    counts, hits, class_hits, cm = got
    tp, n_pred, n_label = counts[:C], counts[C:2 * C], counts[2 * C:3 * C]
    if cm is not None:
        assert np.array_equal(cm.sum(1), n_label) and np.array_equal(cm.sum(0), n_pred) and np.array_equal(np.diag(cm), tp)
    if class_hits is not None and hits is not None:
        assert int(class_hits.sum()) == hits
    if class_hits is not None and k == 1:
        assert np.array_equal(class_hits, tp)


def _labels_at_ranks(x, k, seed):
    """Labels at rank 0, k - 1 and k (a miss where k < C) of their rows in turn, then random ones."""
    B, C = x.shape
    order = _order(x)
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, C, (B,), generator=g).tolist()
    for r in range(min(B, 6)):
        labels[r] = int(order[r, min((0, k - 1, k)[r % 3], C - 1)])
    return labels


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C,k,ld,cmat", SHAPES)
def test_random_rows(lib, B, C, k, ld, cmat, dtype):
    """Random rows with natural ties, labels at rank 0 / k-1 / k; two calls accumulate; the cross-checks between the buffers; and the same
    input through ovmr_eval_counts (all three NULL, k = 1: bit-equal counts) and ovmr_topk_rows (equal hits)."""
    x = _random(B, C, dtype, seed=B * 131 + C)
    labels = _labels_at_ranks(x, k, seed=C)
    want = _want(x, labels, k, cmat)
    buf = Buffers(C, cmat=cmat)
    assert _call(lib, x, labels, k, buf, ld) == 0
    got = buf.host()
    _assert_equal(got, want)
    _identities(got, C, k)
    assert _call(lib, x, labels, k, buf, ld) == 0                       # the second call accumulates
    _assert_equal(buf.host(), want, times=2)
    # the launches it replaces, on the same input
    dev, ld_ = _strided(x, ld)
    lab = torch.as_tensor(labels, dtype=torch.int64).cuda()
    old = torch.zeros(3 * C + 1, dtype=torch.int32, device="cuda")
    assert lib.ovmr_eval_counts(_p(dev), _code(dtype), ld_, _p(lab), B, C, _p(old), _s()) == 0
    bare = Buffers(C, hits=False, class_hits=False, cmat=False)
    assert _call(lib, x, labels, 1, bare, ld) == 0
    assert torch.equal(bare.counts, old)
    hits = torch.zeros(1, dtype=torch.int32, device="cuda")
    idx = torch.zeros((B, k), dtype=torch.int32, device="cuda")
    assert lib.ovmr_topk_rows(_p(dev), _code(dtype), ld_, B, C, k, None, _p(idx), _p(lab), _p(hits), _s()) == 0
    torch.cuda.synchronize()
    assert int(hits.cpu()) == got[1]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C,k,ld", [(5, 65, 5, None), (4, 257, 8, 263), (6, 1000, 5, None)])
def test_ties_and_special_values(lib, B, C, k, ld, dtype):
    """Six values over all columns (ties in every row), an all-equal row, a NaN-only row, a -inf-only row, and the special row of
    test_hip_topk.py (NaN, +-inf, +-0) with its label on -0 / +0 / a NaN in turn."""
    g = torch.Generator().manual_seed(C)
    x = torch.randint(0, 6, (B + 6, C), generator=g).to(dtype)
    x[0] = 0.25
    x[1] = NAN
    x[2] = -INF
    for r in (3, 4, 5):
        x[r] = -INF
        x[r, C - 10:] = torch.tensor(SPECIAL_ROW, dtype=dtype)          # ranks: NaN NaN inf 3 3 3 1 -0 +0 -inf
    labels = _labels_at_ranks(x, k, seed=1)
    labels[0], labels[1], labels[2] = k - 1, k if k < C else 0, 0
    labels[3], labels[4], labels[5] = C - 10 + 4, C - 10 + 5, C - 10 + 7  # -0 (rank 7), +0 (rank 8), the second NaN (rank 1)
    order = _order(x)
    assert order[3, :9].tolist() == [C - 10 + i for i in (1, 7, 6, 2, 3, 9, 0, 4, 5)]
    assert order[:6, 0].tolist() == [0, 0, 0] + [C - 9] * 3             # all-equal / all-NaN / all -inf rows: column 0; the first NaN
    want = _want(x, labels, k)
    assert want[0][C] >= 3 and want[2][k - 1] >= 1                      # the label at column k - 1 of the all-equal row hits
    for nulls in [(True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, True),
                  (False, True, False), (True, False, False), (False, False, False)]:        # every NULL combination
        buf = Buffers(C, *nulls)
        assert _call(lib, x, labels, k, buf, ld) == 0
        got = buf.host()
        _assert_equal(got, want)
        _identities(got, C, k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_labels_outside_the_classes(lib, dtype):
    """Labels -1 and C (and far outside): counted in slot 3C only, no other buffer changes."""
    B, C, k = 5, 65, 5
    x = _random(B, C, dtype, seed=9)
    buf = Buffers(C)
    assert _call(lib, x, [-1, C, -2 ** 40, 2 ** 40, C + 1], k, buf) == 0
    counts, hits, class_hits, cm = buf.host()
    assert counts[3 * C] == B and not counts[:3 * C].any() and hits == 0 and not class_hits.any() and not cm.any()
    labels = [3, -1, C, 3, 64]
    buf = Buffers(C)
    assert _call(lib, x, labels, k, buf) == 0
    _assert_equal(buf.host(), _want(x, labels, k))
    assert buf.host()[0][3 * C] == 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 5])
def test_all_rows_in_one_cell(lib, dtype, k):
    """257 rows with ONE label and ONE prediction (a test pass lists its images class folder by class folder): every sum is exactly 257."""
    B, C = 257, 101
    x = _random(B, C, dtype, seed=17)
    x[:, 40] = 50.0
    hot = 40 if k == 1 else 77
    if k > 1:
        x[:, hot] = 49.0                                                # the label at rank 1
    buf = Buffers(C)
    assert _call(lib, x, [hot] * B, k, buf) == 0
    counts, hits, class_hits, cm = buf.host()
    assert cm[hot, 40] == B and int(cm.sum()) == B
    assert counts[C + 40] == B and counts[2 * C + hot] == B and counts[40] == (B if k == 1 else 0) and counts[3 * C] == 0
    assert int(counts.sum()) == (3 if k == 1 else 2) * B
    assert hits == B and class_hits[hot] == B and int(class_hits.sum()) == B


def test_graph_replay(lib):
    """One launch captured on a single stream and replayed twice: every buffer reads three times the eager result."""
    B, C, k = 6, 1000, 5
    x = _random(B, C, torch.float32, seed=8)
    labels = _labels_at_ranks(x, k, seed=2)
    want = _want(x, labels, k)
    dev, lab = x.cuda(), torch.as_tensor(labels, dtype=torch.int64).cuda()
    buf = Buffers(C)
    args = lambda: (_p(dev), 1, C, _p(lab), B, C, k, _p(buf.counts), _p(buf.hits), _p(buf.class_hits), _p(buf.cmat), _s())     # noqa: E731
    assert lib.ovmr_eval_detail(*args()) == 0
    torch.cuda.synchronize()
    _assert_equal(buf.host(), want)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert lib.ovmr_eval_detail(*args()) == 0
    torch.cuda.synchronize()
    _assert_equal(buf.host(), want)                                     # (capture itself runs nothing)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    _assert_equal(buf.host(), want, times=3)


def test_argument_errors_write_nothing(lib):
    B, C, k = 4, 40, 3
    x = torch.zeros((B, C), device="cuda")
    lab = torch.zeros(B, dtype=torch.int64, device="cuda")
    buf = Buffers(C, fill=POISON)
    s = _s()
    f = lib.ovmr_eval_detail
    rest = (_p(buf.counts), _p(buf.hits), _p(buf.class_hits), _p(buf.cmat), s)
    assert f(None, 1, C, _p(lab), B, C, k, *rest) == -1                 # outputs
    assert f(_p(x), 1, C, None, B, C, k, *rest) == -1                   # labels
    assert f(_p(x), 1, C, _p(lab), B, C, k, None, *rest[1:]) == -1      # counts
    assert f(_p(x), 1, C - 1, _p(lab), B, C, k, *rest) == -1            # ld < C
    assert f(_p(x), 2, C, _p(lab), B, C, k, *rest) == -1                # dtype
    assert f(_p(x), 3, C, _p(lab), B, C, k, *rest) == -1
    assert f(_p(x), 1, C, _p(lab), B, C, 0, *rest) == -1                # k < 1
    assert f(_p(x), 1, C, _p(lab), B, C, 33, *rest) == -1               # k > 32, k <= C
    assert f(_p(x), 1, C, _p(lab), B, C, C + 1, *rest) == -1            # k > C
    assert f(_p(x), 1, 20, _p(lab), B, 20, 21, *rest) == -1             # k > C, k <= 32
    assert f(_p(x), 1, C, _p(lab), -1, C, k, *rest) == -1
    assert f(None, 1, C, None, 0, C, k, None, None, None, None, s) == 0  # B == 0: nothing to do
    assert f(_p(x), 1, C, _p(lab), 0, C, k, *rest) == 0
    torch.cuda.synchronize()
    for t in (buf.counts, buf.hits, buf.class_hits, buf.cmat):
        assert bool((t == POISON).all())


def test_python_binding(lib):
    """runtime.eval_detail: a strided row view without a copy, optional buffers, OvmrError on a refused call."""
    from ovmr_amd import runtime
    x = _random(5, 80, torch.float16, seed=6)
    wide = torch.full((5, 91), NAN, dtype=torch.float16)
    wide[:, 3:83] = x
    view = wide.cuda()[:, 3:83]
    labels = _labels_at_ranks(x, 3, seed=4)
    lab = torch.as_tensor(labels).cuda()
    buf = Buffers(80)
    runtime.eval_detail(view, lab, 3, buf.counts, buf.hits, buf.class_hits, buf.cmat)
    torch.cuda.synchronize()
    _assert_equal(buf.host(), _want(x, labels, 3))
    only = Buffers(80, False, False, False)
    runtime.eval_detail(view, lab, 3, only.counts)
    torch.cuda.synchronize()
    assert torch.equal(only.counts, buf.counts)
    with pytest.raises(runtime.OvmrError):
        runtime.eval_detail(view, lab, 33, buf.counts)
    with pytest.raises(ValueError):
        runtime.eval_detail(view, lab, 3, buf.counts, cmat=torch.zeros(80, dtype=torch.int32, device="cuda"))
