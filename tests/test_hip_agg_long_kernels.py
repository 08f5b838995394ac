"""attn_f32_long (ovmr_amd/csrc/attention.hip) through ovmr_debug_attention_f32_long: fp32 attention over packed sequences of any length,
128-row query tiles walking the keys in order in 64-key LDS blocks -- the kernel the aggregator runs for a chunk whose longest class has
more than 128 rows.  The contract: a row's bits depend on its own sequence alone; for a sequence of at most 128 rows they are the bits
attn_f32_small gives, for a longer one the bits of the same launch on that sequence alone, and max_len, which only sizes the grid,
changes nothing.  Needs an MI355X: run with `pytest -m gpu`.
"""
import pytest
import torch

import attn_exact as A
from agg_long_cases import EXACT, MIXED
from conftest import usable_threads
from test_hip_kernels import _p, _ref_attention, _s
from test_hip_ragged_kernels import CASES, PAD_ROWS, SENTINEL, _inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import runtime
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    torch.set_num_threads(usable_threads())
    return runtime.load_library()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _long(lib, qd, offsets, nseq, n_ctx, max_len, H, rc=0):
    """One launch of the long kernel into a sentinel buffer, PAD_ROWS rows behind the M packed rows; offsets None: the uniform mode."""
    M = qd.shape[0]
    out = torch.empty(M + PAD_ROWS, H * 64, device="cuda")
    out.view(torch.int32).fill_(SENTINEL)
    got = lib.ovmr_debug_attention_f32_long(_p(qd), _p(out), None if offsets is None else _p(offsets), nseq, n_ctx, max_len, H, _s())
    torch.cuda.synchronize()
    assert got == rc, f"rc {got}"
    if rc != 0:
        assert bool((out.view(torch.int32) == SENTINEL).all()), "a refused call launched"
        return None
    assert bool((out[M:].view(torch.int32) == SENTINEL).all()), "wrote behind the last packed row"
    return out[:M]


@pytest.mark.parametrize("kind,L", EXACT, ids=[f"{k}-L{L}" for k, L in EXACT])
def test_long_attention_exact(lib, kind, L):
    """attn_exact's two-level operands (B = H = 3) at the block and tile edges: one bit pattern per element, as test_hip_attn_exact.py
    compares its fp32 cases, the sentinel rows behind M untouched."""
    built = A.build(kind, L, True)
    got = _long(lib, built.qkv.cuda(), None, A.B, 0, L, A.H)
    msg = A.mismatch(got, built.want.cuda(), L)
    assert msg is None, f"{kind}, L = {L}: {msg}"


@pytest.mark.parametrize("case", list(MIXED))
def test_long_mixed_table_launch(lib, case):
    """Short and long sequences in one table launch.  Per sequence: up to 128 rows bit-equal to attn_f32_small on it alone
    (ovmr_debug_attention(1, 0, ...)), beyond that bit-equal to the long kernel's uniform mode on it alone; all within atol 2e-5,
    rtol 1e-4 of the fp64 statement (test_hip_ragged_kernels.py's tolerances: a CPU emulation of the fp32 recurrence on such inputs
    stays below 4.8e-6 absolute at L = 129 / 513 / 1026, the margin the tolerance has at 128).  With every row of every other sequence
    NaN the first, the middle, the last and the shortest sequence keep their bits; nothing is written behind M; and a launch sized for
    640 rows instead of the longest sequence changes no bit.  Prints the largest |got - ref| (DESIGN.md section 4 records it)."""
    H, lens, n_ctx = MIXED[case]
    qkv, row0, offsets = _inputs(H, lens, n_ctx, seed=len(lens) * 100 + H)
    qd = qkv.cuda()
    got = _long(lib, qd, offsets, len(lens), n_ctx, max(lens), H)
    assert bool(torch.isfinite(got).all())
    worst = 0.0
    for b, n in enumerate(lens):
        seq = qd[row0[b]:row0[b + 1]].contiguous()
        if n <= 128:
            alone = torch.empty(n, H * 64, device="cuda")
            assert lib.ovmr_debug_attention(1, 0, _p(seq), _p(alone), 1, n, H, 0, _s()) == 0
            torch.cuda.synchronize()
        else:
            alone = _long(lib, seq, None, 1, 0, n, H)
        mine = got[row0[b]:row0[b + 1]]
        assert torch.equal(_bits(mine), _bits(alone)), f"sequence {b} (length {n}) != the same sequence alone"
        ref = _ref_attention(qkv[row0[b]:row0[b + 1]], 1, n, H, 0)
        worst = max(worst, float((mine.cpu() - ref).abs().max()))
        torch.testing.assert_close(mine.cpu(), ref, atol=2e-5, rtol=1e-4)
    print(f"\n{case}: max |got - fp64 reference| = {worst:.3e}")
    wide = _long(lib, qd, offsets, len(lens), n_ctx, 640, H)
    assert torch.equal(_bits(wide), _bits(got)), "the result depends on max_len"
    for b in sorted({0, len(lens) // 2, len(lens) - 1, lens.index(min(lens))}):
        poisoned = torch.full_like(qd, float("nan"))
        poisoned[row0[b]:row0[b + 1]] = qd[row0[b]:row0[b + 1]]
        again = _long(lib, poisoned, offsets, len(lens), n_ctx, max(lens), H)
        assert torch.equal(_bits(again[row0[b]:row0[b + 1]]), _bits(got[row0[b]:row0[b + 1]])), f"sequence {b} reads its neighbours"


@pytest.mark.parametrize("L", [129, 256, 257])
def test_long_both_modes_on_equal_sequences(lib, L):
    """Three sequences of L rows, two heads: the uniform launch and the table launch on three equal lengths agree bit for bit."""
    H, B = 2, 3
    qkv, _, offsets = _inputs(H, [L] * B, 0, seed=300 + L)
    qd = qkv.cuda()
    table = _long(lib, qd, offsets, B, 0, L, H)
    uniform = _long(lib, qd, None, B, 0, L, H)
    assert torch.equal(_bits(table), _bits(uniform)), "the two modes differ on equal sequences"
    torch.testing.assert_close(uniform.cpu(), _ref_attention(qkv, B, L, H, 0), atol=2e-5, rtol=1e-4)


def test_long_kernel_on_short_launches(lib):
    """The `primary` lengths of test_hip_ragged_kernels.py (all <= 128: one query tile, one or two key blocks) through the long kernel:
    bit-equal to attn_f32_small's table mode."""
    H, lens, n_ctx = CASES["primary"]
    qkv, _, offsets = _inputs(H, lens, n_ctx, seed=len(lens) * 100 + H)
    qd = qkv.cuda()
    M = qd.shape[0]
    small = torch.empty(M, H * 64, device="cuda")
    assert lib.ovmr_debug_attention_f32_varlen(_p(qd), _p(small), _p(offsets), len(lens), n_ctx, max(lens), H, _s()) == 0
    torch.cuda.synchronize()
    got = _long(lib, qd, offsets, len(lens), n_ctx, max(lens), H)
    assert torch.equal(_bits(got), _bits(small))


def test_long_refuses_more_than_4096_rows(lib):
    H = 2
    qkv, _, offsets = _inputs(H, [4, 4], 0, seed=1)
    _long(lib, qkv.cuda(), offsets, 2, 0, 4097, H, rc=-2)
