"""attn_f32_small (ovmr_amd/csrc/attention.hip) in its table mode through ovmr_debug_attention_f32_varlen: fp32 attention over sequences
of different lengths packed row after row, as ovmr_generate_tokens_ragged runs the aggregator.  Per sequence the result must be, bit
for bit, what the kernel's uniform mode (ovmr_debug_attention, f32 = 1: the same body, the starts computed instead of loaded) gives on
that sequence alone, and must not depend on what else is in the launch.  Needs an MI355X: run with `pytest -m gpu`.
"""
import pytest
import torch

from conftest import usable_threads
from test_hip_kernels import _p, _ref_attention, _s

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
PAD_ROWS = 64

# (H, lengths, n_ctx): a sequence of length n is n_ctx context rows + (n - n_ctx) shots, as the offsets array states it
CASES = {
    "primary": (2, [1, 2, 3, 17, 63, 64, 65, 127, 128, 128, 1, 5], 0),    # one row, either side of a wave, the LDS limit twice, short ones behind it
    "eight_heads": (8, [3, 66, 128], 2),
    "twelve_heads": (12, [2, 34], 1),
}


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import runtime
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    torch.set_num_threads(usable_threads())
    return runtime.load_library()


def _inputs(H, lens, n_ctx, seed):
    M = sum(lens)
    qkv = torch.randn(M, 3 * H * 64, generator=torch.Generator().manual_seed(seed))
    row0 = [sum(lens[:b]) for b in range(len(lens) + 1)]
    for b, n in enumerate(lens):                                   # one key row of every sequence scaled x4 (test_hip_strided.py, g)
        qkv[row0[b] + n // 2, H * 64:H * 64 + 64] *= 4.0
    shots = [n - n_ctx for n in lens]
    offsets = torch.tensor([sum(shots[:b]) for b in range(len(lens) + 1)], dtype=torch.int32, device="cuda")
    return qkv, row0, offsets


def _run(lib, qd, offsets, nseq, n_ctx, max_len, H):
    M = qd.shape[0]
    out = torch.empty(M + PAD_ROWS, H * 64, device="cuda")
    out.view(torch.int32).fill_(SENTINEL)
    assert lib.ovmr_debug_attention_f32_varlen(_p(qd), _p(out), _p(offsets), nseq, n_ctx, max_len, H, _s()) == 0
    torch.cuda.synchronize()
    assert bool((out[M:].view(torch.int32) == SENTINEL).all()), "wrote behind the last packed row"
    return out[:M]


@pytest.mark.parametrize("case", list(CASES))
def test_varlen_attention(lib, case):
    """1. bit-equal, sequence by sequence, to the uniform mode on that sequence alone (B = 1, L = len); 2. within the tolerances of
    test_attention_f32_up_to_its_limit of the fp64 statement; 3. the sentinel rows behind M untouched; 4. isolation: with every row of
    every OTHER sequence NaN, a sequence's output keeps its bits; and the launch's max_len (the LDS size) does not change a bit either."""
    H, lens, n_ctx = CASES[case]
    qkv, row0, offsets = _inputs(H, lens, n_ctx, seed=len(lens) * 100 + H)
    qd = qkv.cuda()
    got = _run(lib, qd, offsets, len(lens), n_ctx, max(lens), H)
    assert bool(torch.isfinite(got).all())
    for b, n in enumerate(lens):
        seq = qd[row0[b]:row0[b + 1]].contiguous()
        alone = torch.empty(n, H * 64, device="cuda")
        assert lib.ovmr_debug_attention(1, 0, _p(seq), _p(alone), 1, n, H, 0, _s()) == 0
        torch.cuda.synchronize()
        mine = got[row0[b]:row0[b + 1]]
        assert torch.equal(mine.view(torch.int32), alone.view(torch.int32)), f"sequence {b} (length {n}) != the uniform mode alone"
        ref = _ref_attention(qkv[row0[b]:row0[b + 1]], 1, n, H, 0)
        torch.testing.assert_close(mine.cpu(), ref, atol=2e-5, rtol=1e-4)
    if max(lens) < 128:                                            # 64 KiB of LDS per workgroup: the same bits
        wide = _run(lib, qd, offsets, len(lens), n_ctx, 128, H)
        assert torch.equal(wide.view(torch.int32), got.view(torch.int32)), "the result depends on max_len"
    for b in sorted({0, len(lens) // 2, len(lens) - 1, lens.index(min(lens))}):
        poisoned = torch.full_like(qd, float("nan"))
        poisoned[row0[b]:row0[b + 1]] = qd[row0[b]:row0[b + 1]]
        again = _run(lib, poisoned, offsets, len(lens), n_ctx, max(lens), H)
        assert torch.equal(again[row0[b]:row0[b + 1]].view(torch.int32), got[row0[b]:row0[b + 1]].view(torch.int32)), \
            f"sequence {b} reads its neighbours"


def test_varlen_many_short_sequences(lib):
    """Twenty sequences of 3 to 9 rows, two context rows each: more than one workgroup per head, every start read from the prefix sum.
    Bit-equal to each sequence alone."""
    H, n_ctx = 2, 2
    lens = [3 + (5 * i) % 7 for i in range(20)]
    qkv, row0, offsets = _inputs(H, lens, n_ctx, seed=7)
    qd = qkv.cuda()
    got = _run(lib, qd, offsets, len(lens), n_ctx, 9, H)
    for b, n in enumerate(lens):
        seq = qd[row0[b]:row0[b + 1]].contiguous()
        alone = torch.empty(n, H * 64, device="cuda")
        assert lib.ovmr_debug_attention(1, 0, _p(seq), _p(alone), 1, n, H, 0, _s()) == 0
        torch.cuda.synchronize()
        assert torch.equal(got[row0[b]:row0[b + 1]].view(torch.int32), alone.view(torch.int32)), f"sequence {b} (length {n})"


@pytest.mark.parametrize("L", [1, 64, 65, 128])
def test_both_modes_on_equal_sequences(lib, L):
    """Three sequences of L rows, two heads, through both modes of the kernel: the uniform launch (B = 3) and the table launch on three
    equal lengths (n_ctx = 0) agree bit for bit, both are within the file's tolerances of the fp64 statement, and neither writes
    behind the M = 3 L rows."""
    H, B = 2, 3
    qkv, _, offsets = _inputs(H, [L] * B, 0, seed=300 + L)
    qd = qkv.cuda()
    table = _run(lib, qd, offsets, B, 0, L, H)
    out = torch.empty(B * L + PAD_ROWS, H * 64, device="cuda")
    out.view(torch.int32).fill_(SENTINEL)
    assert lib.ovmr_debug_attention(1, 0, _p(qd), _p(out), B, L, H, 0, _s()) == 0
    torch.cuda.synchronize()
    assert bool((out[B * L:].view(torch.int32) == SENTINEL).all()), "the uniform mode wrote behind the last row"
    uniform = out[:B * L]
    assert torch.equal(table.view(torch.int32), uniform.view(torch.int32)), "the two modes differ on equal sequences"
    ref = _ref_attention(qkv, B, L, H, 0)
    torch.testing.assert_close(uniform.cpu(), ref, atol=2e-5, rtol=1e-4)
    torch.testing.assert_close(table.cpu(), ref, atol=2e-5, rtol=1e-4)


def test_varlen_refuses_more_than_128_rows(lib):
    H = 2
    qkv, _, offsets = _inputs(H, [4, 4], 0, seed=1)
    qd = qkv.cuda()
    out = torch.empty(8 + PAD_ROWS, H * 64, device="cuda")
    out.view(torch.int32).fill_(SENTINEL)
    assert lib.ovmr_debug_attention_f32_varlen(_p(qd), _p(out), _p(offsets), 2, 0, 129, H, _s()) == -2
    torch.cuda.synchronize()
    assert bool((out.view(torch.int32) == SENTINEL).all()), "a refused call launched"
