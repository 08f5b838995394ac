"""The attention kernels held to exact values: every case of attn_exact.CASES -- one-hot permutations, shared-code groups, causal groups and
uniform weights, at the lengths where a kernel changes its path -- on operands whose scores have two levels, so that the output row is the
plain mean of the addressed V rows: ONE fp16 bit pattern whatever the kernel's block order, reference maximum or row-sum form
(attn_exact.py: the method and the case table; test_attn_exact_cpu.py: the builder keeps its promises and the fp64 reference agrees).
For every case and every variant of its row of the table

  * the output equals the expected tensor element for element (torch.equal on fp16; == on every element for the fp32 kernel);
  * the output buffer is filled with a sentinel, PAD_ROWS rows behind it: they stay untouched;
  * through ovmr_debug_attention_q the first Lq rows of every sequence equal the same expected rows.

The lazily moved reference maximum of variants 1 and 5 is the one path two score levels cannot reach: test_attention_three_levels holds it
to a derived bound.  On a mismatch the message gives the count, the queries, the first (sequence, query, head, column), got against want.
Needs an MI355X: run with `pytest -m gpu`.
"""
import ctypes

import pytest
import torch

import attn_exact as A
from conftest import usable_threads
from test_hip_kernels import _ref_attention

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import runtime
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    torch.set_num_threads(usable_threads())
    return runtime.load_library()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _launch(lib, variant, qkv, L, Lq, causal, f32=False):
    """One launch into a sentinel buffer with PAD_ROWS rows behind the output; returns the output rows [B * Lq, H * 64]."""
    rows = A.B * Lq
    out = A.sentinel_buffer(rows + A.PAD_ROWS, A.H * 64, qkv.dtype, "cuda")
    if Lq != L:
        rc = lib.ovmr_debug_attention_q(variant, _p(qkv), _p(out), A.B, L, Lq, A.H, causal, _s())
    else:
        rc = lib.ovmr_debug_attention(int(f32), variant, _p(qkv), _p(out), A.B, L, A.H, causal, _s())
    assert rc == 0, f"rc {rc}"
    torch.cuda.synchronize()
    assert A.untouched(out[rows:]), "wrote behind the last output row"
    return out[:rows]


@pytest.mark.parametrize("c", A.CASES, ids=lambda c: c.id)
def test_attention_exact(lib, c):
    built = A.build(c.kind, c.L, c.f32)
    qkv, want = built.qkv.cuda(), built.want.cuda()
    bad = []
    for variant in c.variants or (0,):
        msg = A.mismatch(_launch(lib, variant, qkv, c.L, c.L, c.causal, c.f32), want, c.L)
        if msg is not None:
            bad.append(f"{c.id}, {'fp32 kernel' if c.f32 else f'variant {variant}'}: {msg}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind", ["onehot", "uniform"])
@pytest.mark.parametrize("L", A.Q_L)
def test_attention_q_exact(lib, L, kind):
    """ovmr_debug_attention_q: the first Lq in {1, 16, 17, 33} queries of every sequence (the CLS-only launch of the last vision block, ragged
    16-row tiles of variants 0 / 1, variant 5 from Lq = 32 on) against the same expected rows; the one-hot permutation puts the edge keys --
    L - 1, the tail block, the last full block, key 0 -- on the first queries, another one first per (sequence, head)."""
    built = A.build(kind, L)
    qkv = built.qkv.cuda()
    for Lq in A.Q_LQ:
        want = built.want.view(A.B, L, -1)[:, :Lq].reshape(A.B * Lq, -1).cuda()
        for variant in A.ATTN_VARIANTS:
            msg = A.mismatch(_launch(lib, variant, qkv, L, Lq, 0), want, Lq)
            assert msg is None, f"{kind}, L = {L}, Lq = {Lq}, variant {variant}: {msg}"


@pytest.mark.parametrize("L", A.THREE_L)
def test_attention_three_levels(lib, L):
    """Three score levels per row (attn_exact.three_level): the match, a key 5.77 below it in the log2 domain -- under the threshold of 8, so
    that the reference maximum of variants 1 and 5 stays stale and P of the match is about 54 -- and a key 11.5 below, for which the reference
    moves and alpha is applied; in all six orders over three key blocks and once in one block, the same order for all rows of a 32-row tile.
    Variant 0 and, at L = 197, variant 3 take the exact maximum and must agree.  Expected: the fp64 reference rounded to fp16;
    |got - ref| <= 3 * 2^-10, derived, not measured:
      * the scores are exact integers (1024, 992, 960, and 768 at most for every other key);
      * P rounded to fp16 carries a relative error of at most 2^-11 per key, whatever reference it is taken against (P <= 2^8 stays normal);
      * the row sum is taken from the rounded P in variants 1 and 3 and from the unrounded P in variants 0 and 5, the numerator from the
        rounded P in all of them;
      * V lies in [1, 2), all positive: no cancellation, so numerator and denominator together move the quotient by at most 2^-10 relative,
        which is under 2 steps of 2^-10 at values below 2;
      * half a step for the final rounding of the output, and the reference's own rounding is the value compared against;
      * v_exp_f32's error (about 2^-22) and the P of far keys that goes subnormal in fp16 contribute under 0.05 step at L = 577.
    That is 2 + 0.5 + 0.05 steps: 3 * 2^-10 holds them."""
    three = A.three_level(L)
    ref = _ref_attention(three.qkv.float(), A.B, L, A.H, 0).half().float().cuda()
    assert float(ref.min()) >= 1.0 and float(ref.max()) < 2.0
    qkv = three.qkv.cuda()
    for variant in (0, 1, 5) + ((3,) if L == 197 else ()):
        got = _launch(lib, variant, qkv, L, L, 0).float()
        err = (got - ref).abs()
        assert bool(torch.isfinite(got).all())
        assert float(err.max()) <= 3 * 2.0 ** -10, f"L = {L}, variant {variant}: max |got - ref| = {float(err.max()) * 1024:.3f} * 2^-10"
