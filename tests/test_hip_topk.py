"""ovmr_topk_rows (csrc/topk.hip) at the C ABI, through ctypes.  The expected indices are ALWAYS those of the stable descending sort on the
CPU, torch.sort(x.float(), dim=1, descending=True, stable=True)[1][:, :k] -- larger value first, equal values in increasing column order,
NaN above +inf, -0 == +0 -- and the expected values x.float() gathered there, compared bit for bit (NaN positions as a mask).  Every case
runs in fp16 and fp32.  Run with -m gpu on an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
SPECIAL_ROW = [1, NAN, 3, 3, -0.0, 0.0, INF, NAN, -INF, 3]
DTYPES = [torch.float16, torch.float32]
# (B, C, k, ld): the smallest call; k = C with B no multiple of a block's four rows; the lane boundary; rows that are not 16-byte aligned
# (the scalar path) and C no multiple of the vector width; aligned rows with the largest k and a scalar tail; several blocks; the c1 vocabulary
SHAPES = [(1, 1, 1, None), (3, 7, 7, None), (5, 63, 5, None), (5, 64, 5, None), (5, 65, 5, None), (4, 257, 8, 263), (4, 264, 32, 264),
          (6, 1000, 5, None), (2, 21841, 10, None)]


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


def _want(x, k):
    xf = x.float()
    idx = torch.sort(xf, dim=1, descending=True, stable=True)[1][:, :k]
    return idx, xf.gather(1, idx)


def _same_bits(got, want):
    got, want = got.cpu(), want.cpu()
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(got.view(torch.int32)[~nan], want.view(torch.int32)[~nan])


def _call(lib, x, k, ld=None, labels=None, hits=None, values=True):
    dev, ld = _strided(x, ld)
    B, C = x.shape
    idx = torch.full((B, k), -7, dtype=torch.int32, device="cuda")
    val = torch.full((B, k), -7.0, dtype=torch.float32, device="cuda") if values else None
    rc = lib.ovmr_topk_rows(_p(dev), _code(x.dtype), ld, B, C, k, _p(val), _p(idx), _p(labels), _p(hits), _s())
    torch.cuda.synchronize()
    return rc, val, idx


def _check(lib, x, k, ld=None):
    rc, val, idx = _call(lib, x, k, ld)
    assert rc == 0
    want_idx, want_val = _want(x, k)
    assert torch.equal(idx.cpu().long(), want_idx), f"indices differ from the stable sort: {idx.cpu()[:2]} vs {want_idx[:2]}"
    assert _same_bits(val, want_val)
    return idx


def _random(B, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, C), generator=g).half().to(dtype)           # fp16-rounded normals: ties occur naturally


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C,k,ld", SHAPES)
def test_random_rows_equal_the_stable_sort(lib, B, C, k, ld, dtype):
    x = _random(B, C, dtype, seed=B * 131 + C)
    _check(lib, x, k, ld)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C,k,ld", [s for s in SHAPES if s[1] >= 7])
def test_ties_nan_and_infinities(lib, B, C, k, ld, dtype):
    """Row 0 all equal (columns 0..k-1); row 1 one value repeated in columns of different lanes and of the scalar tail, above everything
    else; row 2 only NaN; a further row only -inf; the rest random."""
    x = _random(max(B, 4), C, dtype, seed=C + 5)
    x[0] = 0.25
    rep = sorted({0, 1, C // 3, C // 2, C - 2, C - 1} | ({63, 64, 65, 130} & set(range(C))))
    x[1] = -1.0
    x[1, rep] = 9.0
    x[2] = NAN
    x[3] = -INF
    idx = _check(lib, x, k, ld).cpu()
    assert idx[0].tolist() == list(range(k)) and idx[2].tolist() == list(range(k)) and idx[3].tolist() == list(range(k))
    assert idx[1].tolist() == (rep + [c for c in range(C) if c not in rep])[:k]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_special_row(lib, dtype):
    x = torch.full((2, 65), -INF, dtype=dtype)
    x[0, :10] = torch.tensor(SPECIAL_ROW, dtype=dtype)
    x[1, 55:] = torch.tensor(SPECIAL_ROW, dtype=dtype)                  # the same values across the lane boundary
    for ld in (None, 67):
        idx = _check(lib, x, 11, ld).cpu()
        assert idx[0].tolist() == [1, 7, 6, 2, 3, 9, 0, 4, 5, 8, 10]
        assert idx[1].tolist() == [56, 62, 61, 57, 58, 64, 55, 59, 60, 0, 1]
    rc, val, _ = _call(lib, x, 11)
    v = val.cpu()[0]
    assert torch.isnan(v[:2]).all() and v[2] == INF and v[7:9].view(torch.int32).tolist() == [-2 ** 31, 0]    # -0 keeps its sign, then +0
    assert v[9] == -INF


def _distinct(B, C, dtype, seed):
    """B rows, each a permutation of C distinct finite fp16 bit patterns (no -0: it equals +0)."""
    bits = np.array([b for b in range(0x10000) if (b & 0x7C00) != 0x7C00 and b != 0x8000], dtype=np.uint16)
    assert len(bits) >= C
    rng = np.random.default_rng(seed)
    rows = np.stack([rng.permutation(bits)[:C] for _ in range(B)])
    return torch.from_numpy(rows.view(np.float16).copy()).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C,k,ld", SHAPES)
def test_distinct_values_equal_torch_topk(lib, B, C, k, ld, dtype):
    """torch.topk is a valid reference only where no tie exists."""
    x = _distinct(B, C, dtype, seed=C)
    idx = _check(lib, x, k, ld)
    rc, val, _ = _call(lib, x, k, ld)
    tv, ti = torch.topk(x.float(), k, dim=1)
    assert torch.equal(idx.cpu().long(), ti) and torch.equal(val.cpu(), tv)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rank_zero_is_the_evaluators_prediction(lib, dtype):
    """indices[:, 0] implies the n_pred histogram ovmr_eval_counts builds on the same matrix, ties and NaN rows included."""
    B, C, k = 11, 65, 3
    x = _random(B, C, dtype, seed=2)
    x[0] = 0.5
    x[1, 7] = x[1, 40] = 30.0
    x[2, 64] = x[2, 63] = 30.0
    x[3, 50] = NAN
    x[3, 9] = NAN
    x[4] = NAN
    x[5] = -INF
    x[6, :10] = torch.tensor(SPECIAL_ROW, dtype=dtype)
    x[7, 3], x[7, 2] = 0.0, -0.0
    x[7, 4:] = -1.0
    x[7, :2] = -2.0
    idx = _check(lib, x, k, 71)
    dev, ld = _strided(x, 71)
    counts = torch.zeros(3 * C + 1, dtype=torch.int32, device="cuda")
    lab = torch.zeros(B, dtype=torch.int64, device="cuda")
    assert lib.ovmr_eval_counts(_p(dev), _code(dtype), ld, _p(lab), B, C, _p(counts), _s()) == 0
    torch.cuda.synchronize()
    assert torch.equal(counts[C:2 * C].cpu().long(), torch.bincount(idx[:, 0].cpu().long(), minlength=C))
    assert idx[:, 0].cpu().tolist()[:8] == [0, 7, 63, 9, 0, 0, 1, 2]


@pytest.mark.parametrize("dtype", DTYPES)
def test_hits(lib, dtype):
    B, C, k = 10, 257, 8
    x = _random(B, C, dtype, seed=4)
    order = torch.sort(x.float(), dim=1, descending=True, stable=True)[1]
    ranks = [0, k - 1, k, 0, k - 1, k, 3, C - 1]                        # label at rank 0, at rank k-1, at rank k (a miss), ...
    labels = [int(order[r, ranks[r]]) for r in range(8)] + [-1, C]      # ... and outside [0, C): never a hit
    want = sum(r < k for r in ranks)
    lab = torch.tensor(labels, dtype=torch.int64, device="cuda")
    hits = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc, val, idx = _call(lib, x, k, 263, lab, hits)
    assert rc == 0 and int(hits.cpu()) == want == 5
    rc, none, idx2 = _call(lib, x, k, 263, lab, hits, values=False)     # a second call accumulates; values = NULL
    assert rc == 0 and none is None and int(hits.cpu()) == 2 * want
    assert torch.equal(idx, idx2) and torch.equal(idx.cpu().long(), order[:, :k])


def test_graph_replay(lib):
    """One call captured on a single stream and replayed twice: hits = three times the eager count, the indices unchanged."""
    B, C, k = 6, 1000, 5
    x = _random(B, C, torch.float32, seed=8)
    order = torch.sort(x, dim=1, descending=True, stable=True)[1]
    lab = torch.stack([order[0, 0], order[1, k - 1], order[2, k], order[3, 2], order[4, 900], order[5, 1]]).cuda()
    dev = x.cuda()
    hits = torch.zeros(1, dtype=torch.int32, device="cuda")
    idx = torch.zeros((B, k), dtype=torch.int32, device="cuda")
    val = torch.zeros((B, k), dtype=torch.float32, device="cuda")
    args = lambda: (_p(dev), 1, C, B, C, k, _p(val), _p(idx), _p(lab), _p(hits), _s())     # noqa: E731
    assert lib.ovmr_topk_rows(*args()) == 0
    torch.cuda.synchronize()
    eager, eager_idx = int(hits.cpu()), idx.clone()
    assert eager == 4
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert lib.ovmr_topk_rows(*args()) == 0
    torch.cuda.synchronize()
    captured = int(hits.cpu())                                         # (capture itself runs nothing)
    assert captured == eager
    idx.zero_()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert int(hits.cpu()) == 3 * eager
    assert torch.equal(idx, eager_idx) and torch.equal(idx.cpu().long(), order[:, :k])


def test_argument_errors_write_nothing(lib):
    B, C, k = 4, 40, 3
    x = torch.zeros((B, C), device="cuda")
    idx = torch.full((B, 33), -7, dtype=torch.int32, device="cuda")
    val = torch.full((B, 33), -7.0, device="cuda")
    lab = torch.zeros(B, dtype=torch.int64, device="cuda")
    hits = torch.zeros(1, dtype=torch.int32, device="cuda")
    s = _s()
    f = lib.ovmr_topk_rows
    assert f(None, 1, C, B, C, k, _p(val), _p(idx), None, None, s) == -1              # outputs
    assert f(_p(x), 1, C, B, C, k, _p(val), None, None, None, s) == -1                # indices
    assert f(_p(x), 1, C, B, C, 0, _p(val), _p(idx), None, None, s) == -1             # k < 1
    assert f(_p(x), 1, C, B, C, C + 1, _p(val), _p(idx), None, None, s) == -1         # k > C (and > 32)
    assert f(_p(x), 1, C, B, C, 33, _p(val), _p(idx), None, None, s) == -1            # k > 32, k <= C
    assert f(_p(x), 1, 20, B, 20, 21, _p(val), _p(idx), None, None, s) == -1          # k > C, k <= 32
    assert f(_p(x), 1, C - 1, B, C, k, _p(val), _p(idx), None, None, s) == -1         # ld < C
    assert f(_p(x), 2, C, B, C, k, _p(val), _p(idx), None, None, s) == -1             # dtype
    assert f(_p(x), 3, C, B, C, k, _p(val), _p(idx), None, None, s) == -1
    assert f(_p(x), 1, C, B, C, k, _p(val), _p(idx), _p(lab), None, s) == -1          # labels without hits
    assert f(_p(x), 1, C, B, C, k, _p(val), _p(idx), None, _p(hits), s) == -1         # hits without labels
    assert f(_p(x), 1, C, -1, C, k, _p(val), _p(idx), None, None, s) == -1
    assert f(None, 1, C, 0, C, k, None, None, None, None, s) == 0                     # B == 0: nothing to do
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((val == -7.0).all()) and int(hits.cpu()) == 0


def test_python_binding(lib):
    """runtime.topk_rows: a strided row view without a copy, labels / hits, OvmrError on a refused call."""
    from ovmr_amd import runtime
    x = _random(5, 80, torch.float16, seed=6)
    wide = torch.full((5, 91), NAN, dtype=torch.float16)
    wide[:, 3:83] = x
    view = wide.cuda()[:, 3:83]
    order = torch.sort(x.float(), dim=1, descending=True, stable=True)[1]
    lab = order[:, 2].contiguous().cuda()
    hits = torch.zeros(1, dtype=torch.int32, device="cuda")
    val, idx = runtime.topk_rows(view, 3, lab, hits)
    assert val.dtype == torch.float32 and idx.dtype == torch.int32 and val.shape == idx.shape == (5, 3)
    assert torch.equal(idx.cpu().long(), order[:, :3]) and torch.equal(val.cpu(), x.float().gather(1, order[:, :3]))
    assert int(hits.cpu()) == 5
    with pytest.raises(runtime.OvmrError):
        runtime.topk_rows(view, 33)
    with pytest.raises(ValueError):
        runtime.topk_rows(view, 3, lab, None)
