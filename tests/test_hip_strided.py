"""Kernel parity of the engine's sub-matrix launches -- strided GEMM operands and attention for a subset of the queries -- through
ovmr_debug_gemm_strided / ovmr_debug_attention_q, against the fp64 statements of test_hip_kernels.py with its rounding points and
tolerances.  Every case also fills its output with a sentinel bit pattern and asserts, bit for bit, that nothing outside the written
rows and columns changed.  Needs an MI355X: run with `pytest -m gpu`.

a. CLS-row Q projection: A strided by a sequence (lda = L*W), C by L*3W, and the folded form reading the LayerNorm statistics every
   L rows (ln_stride) -- ovmr_amd/csrc/ovmr_api.hip, the second part of the last block's in_proj in run_block_f16 (ln_linear: folded and plain).
b. K/V projection written next to Q: W and bias offset by W rows, C = qkv + W with N = 2W, ldc = 3W -- its first part.
c. out_proj of the CLS rows: residual read from the token rows (ldres = L*W), C a separate [Bc, W] -- run_block_f16 with cls_rows.
d. logits with odd and padded ldc (N = classes, rows not 16-byte aligned) -- the head GEMMs of ovmr_fused_logits and ovmr_zeroshot_logits.
e. A strided near the v5 kernel's 32-bit offset guard (gemm_f16_v5.hip:817-820): the last rows of both sides of M * lda * 2 = 2^31.
f. attention for the first Lq < L queries (Lq = 1: the CLS query) -- launch_attention_f16_q in run_block_f16 with cls_rows.
g. fp32 aggregator attention up to its L <= 128 limit (64 KiB of dynamic LDS) -- run_block_f32, run by ovmr_generate_tokens.
"""
import pytest
import torch

from conftest import usable_threads
from test_hip_kernels import (EPI_BIAS, EPI_BIAS_RES, EPI_NONE, EPI_SCALE, GEMM_VARIANTS, ATTN_VARIANTS, _h, _p, _ref_attention,
                              _ref_gemm_f16, _s)

pytestmark = pytest.mark.gpu

EPI_LN_BIAS = 6
SENTINEL = 0x5A5A                       # fp16 203.25: a finite value no kernel output here takes by chance, compared as bits
PAD_ROWS = 64                           # sentinel rows behind every output: a store past the last row lands there
STRIDED_VARIANTS = GEMM_VARIANTS + [7]  # 7: the tile kernels without the split-K one -- what the engine's plain K/V and Q launches take


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import runtime
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    torch.set_num_threads(usable_threads())
    return runtime.load_library()


def _sentinel(rows, cols):
    t = torch.empty((rows, cols), dtype=torch.float16, device="cuda")
    t.view(torch.int16).fill_(SENTINEL)
    return t


def _untouched(t):
    return bool((t.view(torch.int16) == SENTINEL).all())


def _gemm_strided(lib, variant, A, lda, W, ldw, bias, res, ldres, C, ldc, M, N, K, epi, scale=1.0, gamma=None, beta=None, row_step=1):
    return lib.ovmr_debug_gemm_strided(variant, _p(A), lda, _p(W), ldw, _p(bias), _p(res), ldres, _p(C), ldc, M, N, K, epi, scale,
                                       _p(gamma), _p(beta), row_step, _s())


def _assert_gemm_close(got, ref, what):
    """test_gemm_f16's bar: one fp16 ulp of the largest magnitude, and few elements beyond an eighth of it."""
    tol = 2e-3 * max(1.0, float(ref.abs().max()))
    assert torch.isfinite(got).all(), what
    assert float((got - ref).abs().max()) <= tol, f"{what}: max err {(got - ref).abs().max()}"
    assert float(((got - ref).abs() > tol / 8).float().mean()) < 0.02, what


def _assert_ln_close(got, x, gamma, beta, Wt, b, what):
    """test_gemm_layernorm_fold's bars: as close to the unrounded fp64 LayerNorm-then-Linear as the reference's own fp16 path is,
    within 4e-3 of that path, and 1 - cos < 1e-5 per row."""
    D = x.shape[1]
    ln64 = torch.nn.functional.layer_norm(x.double(), (D,), gamma.double(), beta.double(), 1e-5)
    ln16 = _h(torch.nn.functional.layer_norm(x.float(), (D,), gamma, beta, 1e-5))
    exact = ln64 @ Wt.double().t() + b.double()
    ref = _h((ln16.double() @ Wt.double().t() + b.double()).float())
    assert torch.isfinite(got).all(), what
    err_got = float((got.double() - exact).pow(2).mean().sqrt())
    err_ref = float((ref.double() - exact).pow(2).mean().sqrt())
    assert err_got <= 1.25 * err_ref + 1e-5, f"{what}: folded rms error {err_got:.3e} vs reference path {err_ref:.3e}"
    tol = 4e-3 * max(1.0, float(ref.abs().max()))
    assert float((got - ref).abs().max()) <= tol, f"{what}: max err {(got - ref).abs().max()}"
    cos = torch.nn.functional.cosine_similarity(got, ref, dim=1)
    assert float((1 - cos).max()) < 1e-5, what


def _residual_stream(rows, W, seed):
    """fp16 token rows with an outlier channel and per-channel offsets (non-zero row means), as test_gemm_layernorm_fold's residual:
    a LayerNorm row that reads another row's statistics is far off.  Generated on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((rows, W), generator=g, device="cuda")
    x[:, 5] *= 20.0
    x += torch.randn(W, generator=g, device="cuda") * 0.5
    return x.half()


def _in_proj(W, seed):
    g = torch.Generator().manual_seed(seed)
    Wt = (torch.randn(3 * W, W, generator=g) * W ** -0.5).half()
    b = (torch.randn(3 * W, generator=g) * 0.1).half()
    gamma, beta = 1.0 + 0.3 * torch.randn(W, generator=g), 0.2 * torch.randn(W, generator=g)
    return Wt, b, gamma, beta


def _sample_rows(M, seed):
    """The first rows, the last 300 (the ragged last 64- and 256-row tiles), rows on tile borders, a few random ones."""
    idx = set(range(min(M, 64))) | set(range(max(0, M - 300), M))
    for t in (64, 128, 256, 512, 1024, 4096):
        for k in range(t, M, t * max(1, M // (8 * t))):
            idx |= {r for r in (k - 1, k) if 0 <= r < M}
    idx |= set(torch.randint(0, M, (32,), generator=torch.Generator().manual_seed(seed)).tolist())
    return torch.tensor(sorted(idx))


# ---- a. CLS-row Q projection -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Bc", [256, 300, 775])
@pytest.mark.parametrize("W,L", [(768, 50), (768, 197), (1024, 257), (1024, 577)])
def test_cls_row_q_projection(lib, W, L, Bc):
    """Q of the CLS rows only: A = x strided by a sequence (lda = L*W), C = qkv strided by L*3W -- against fp64, bit-equal to the
    same variant on the gathered contiguous rows (same kernel, same K order); the folded form (epi 6) reads the statistics of every
    L-th token row (ln_stride = L * W/256) and is bit-equal to ovmr_debug_lnfold on the gathered rows.  Nothing but the Q columns
    of the CLS rows is written: the token rows in between, the K/V columns and the rows behind stay sentinel."""
    M = Bc * L
    x = _residual_stream(M, W, W + L + Bc)
    xc = x.view(Bc, L, W)[:, 0].contiguous()                # the CLS rows, gathered
    xc_h = xc.float().cpu()
    Wt, b, gamma, beta = _in_proj(W, W + L)
    Wd, bd, gd, betad = Wt.cuda(), b.cuda(), gamma.cuda(), beta.cuda()
    ref = _ref_gemm_f16(xc_h, Wt[:W], b[:W], None, None, EPI_BIAS, 1.0, 0, 0)
    qkv = _sentinel(M + PAD_ROWS, 3 * W)

    def written(what):
        rows = qkv[:M].view(Bc, L, 3 * W)
        assert _untouched(rows[:, 0, W:]) and _untouched(rows[:, 1:]) and _untouched(qkv[M:]), f"{what}: wrote outside the Q block"
        return rows[:, 0, :W].clone()

    for variant in STRIDED_VARIANTS:
        qkv.view(torch.int16).fill_(SENTINEL)
        assert _gemm_strided(lib, variant, x, L * W, Wd, W, bd, None, 0, qkv, L * 3 * W, Bc, W, W, EPI_BIAS) == 0
        gath = _sentinel(Bc + PAD_ROWS, W)
        assert lib.ovmr_debug_gemm(0, variant, _p(xc), _p(Wd), _p(bd), None, None, _p(gath), Bc, W, W, W, EPI_BIAS, 1.0, 0, 0, _s()) == 0
        torch.cuda.synchronize()
        got = written(f"variant {variant}")
        _assert_gemm_close(got.float().cpu(), ref, f"variant {variant}")
        assert torch.equal(got.view(torch.int16), gath[:Bc].view(torch.int16)), f"variant {variant}: strided != gathered"
        assert _untouched(gath[Bc:])
    for variant in (6, 8):                                  # the LN-folding epilogues run on the 256-row tile kernels only
        qkv.view(torch.int16).fill_(SENTINEL)
        assert _gemm_strided(lib, variant, x, L * W, Wd, W, bd, None, 0, qkv, L * 3 * W, Bc, W, W, EPI_LN_BIAS,
                             gamma=gd, beta=betad, row_step=L) == 0
        gath = _sentinel(Bc + PAD_ROWS, W)
        assert lib.ovmr_debug_lnfold(variant, None, None, None, None, Bc, W, 0, _p(Wd), _p(gd), _p(betad), _p(bd), W, 0,
                                     _p(xc), _p(gath), _s()) == 0
        torch.cuda.synchronize()
        got = written(f"folded, variant {variant}")
        _assert_ln_close(got.float().cpu(), xc_h, gamma, beta, Wt[:W], b[:W], f"folded, variant {variant}")
        assert torch.equal(got.view(torch.int16), gath[:Bc].view(torch.int16)), f"folded, variant {variant}: strided != gathered"


# ---- b. K/V next to Q --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,L,Bc", [(768, 197, 3), (1024, 257, 1),            # M = 591 / 257: the split-K kernel's shapes under 8
                                    (768, 197, 37), (1024, 257, 5),           # M = 7289 / 1285: tile kernels, ragged last tiles
                                    (768, 50, 256)])                          # M = 12800: a batch-256 launch of ViT-B/32
def test_kv_projection_into_the_column_offset(lib, W, L, Bc):
    """K and V of every token into columns W..3W of qkv: W and bias offset by W rows, C = qkv + W, N = 2W, ldc = 3W, plain (EPI_BIAS)
    and folded (epi 6, statistics of every row).  fp64 on sampled rows (first, last / ragged, tile borders); the Q columns and the
    rows behind stay sentinel over the whole buffer."""
    M = Bc * L
    x = _residual_stream(M, W, 7 * W + M)
    Wt, b, gamma, beta = _in_proj(W, W + M)
    Wd, bd, gd, betad = Wt.cuda(), b.cuda(), gamma.cuda(), beta.cuda()
    rows = _sample_rows(M, M)
    xs = x[rows.cuda()].float().cpu()
    ref = _ref_gemm_f16(xs, Wt[W:], b[W:], None, None, EPI_BIAS, 1.0, 0, 0)
    qkv = _sentinel(M + PAD_ROWS, 3 * W)
    for epi in (EPI_BIAS, EPI_LN_BIAS):
        for variant in STRIDED_VARIANTS:
            what = f"epi {epi}, variant {variant}"
            qkv.view(torch.int16).fill_(SENTINEL)
            kw = dict(gamma=gd, beta=betad, row_step=1) if epi == EPI_LN_BIAS else {}
            assert _gemm_strided(lib, variant, x, W, Wd[W:], W, bd[W:], None, 0, qkv[:, W:], 3 * W, M, 2 * W, W, epi, **kw) == 0
            torch.cuda.synchronize()
            assert _untouched(qkv[:M, :W]) and _untouched(qkv[M:]), f"{what}: wrote outside the K/V columns"
            got = qkv[rows.cuda(), W:].float().cpu()
            if epi == EPI_BIAS:
                _assert_gemm_close(got, ref, what)
            else:
                _assert_ln_close(got, xs, gamma, beta, Wt[W:], b[W:], what)
            assert bool(torch.isfinite(qkv[:M, W:]).all()), f"{what}: unwritten K/V elements"


# ---- c. out_proj with the residual strided over the token rows ------------------------------------------------------------------

@pytest.mark.parametrize("Bc", [37, 256, 775, 1345])     # 1345: variant 8 takes the 256-row tile kernel (not a latency-bound shape)
@pytest.mark.parametrize("W,L", [(768, 197), (1024, 257)])
def test_out_proj_residual_from_the_token_rows(lib, W, L, Bc):
    """rows = h(h(yc Wo^T + bo) + x[CLS rows]): the residual read from the token buffer with ldres = L*W, not in place; C a separate
    [Bc, W] (ldc = W).  x stays untouched, nothing is written behind the Bc rows."""
    x = _residual_stream(Bc * L, W, 3 * W + L + Bc)
    x_before = x.clone()
    g = torch.Generator().manual_seed(W + Bc)
    yc = (torch.randn(Bc, W, generator=g) * 0.5).half()
    Wo = (torch.randn(W, W, generator=g) * W ** -0.5).half()
    bo = (torch.randn(W, generator=g) * 0.1).half()
    ref = _ref_gemm_f16(yc, Wo, bo, x.view(Bc, L, W)[:, 0].float().cpu(), None, EPI_BIAS_RES, 1.0, 0, 0)
    ycd, Wod, bod = yc.cuda(), Wo.cuda(), bo.cuda()
    out = _sentinel(Bc + PAD_ROWS, W)
    for variant in GEMM_VARIANTS:
        out.view(torch.int16).fill_(SENTINEL)
        assert _gemm_strided(lib, variant, ycd, W, Wod, W, bod, x, L * W, out, W, Bc, W, W, EPI_BIAS_RES) == 0
        torch.cuda.synchronize()
        assert _untouched(out[Bc:]), f"variant {variant}: wrote behind the last row"
        assert torch.equal(x.view(torch.int16), x_before.view(torch.int16)), f"variant {variant}: the residual was written"
        _assert_gemm_close(out[:Bc].float().cpu(), ref, f"variant {variant}")


# ---- d. unaligned and padded ldc ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pad", [0, 8, 1])
@pytest.mark.parametrize("N", [6, 1003, 21841])
def test_gemm_odd_and_padded_ldc(lib, N, pad):
    """Logits with N = classes and ldc = N, N + 8, N + 1 (rows that are not 16-byte aligned), M in {1, 64, 256, 257}, EPI_NONE and
    EPI_SCALE: every variant runs correctly or returns an error code, and never writes the padding columns or behind the last row."""
    K, Mmax, ldc = 512, 257, N + pad
    g = torch.Generator().manual_seed(N + pad)
    A = (torch.randn(Mmax, K, generator=g) * 0.5).half()
    Wt = (torch.randn(N, K, generator=g) * K ** -0.5).half()
    Ad, Wd = A.cuda(), Wt.cuda()
    for epi in (EPI_NONE, EPI_SCALE):
        ref_all = _ref_gemm_f16(A, Wt, None, None, None, epi, 100.0, 0, 0)
        for M in (1, 64, 256, 257):
            C = _sentinel(M + PAD_ROWS, ldc)
            for variant in GEMM_VARIANTS:
                what = f"epi {epi}, M {M}, variant {variant}"
                C.view(torch.int16).fill_(SENTINEL)
                rc = _gemm_strided(lib, variant, Ad, K, Wd, K, None, None, 0, C, ldc, M, N, K, epi, scale=100.0)
                torch.cuda.synchronize()
                assert _untouched(C[M:]) and _untouched(C[:M, N:]), f"{what}: wrote outside [M, N] (rc {rc})"
                if rc != 0:
                    assert _untouched(C), f"{what}: rc {rc} but C was written"
                    continue
                _assert_gemm_close(C[:M, :N].float().cpu(), ref_all[:M], what)


# ---- e. A strided across the 32-bit offset guard of the tile kernel ---------------------------------------------------------------

@pytest.mark.parametrize("M", [7096, 7098])
def test_gemm_strided_a_near_the_32bit_offset_guard(lib, M):
    """lda = 197 * 768 (a CLS-row launch): M = 7096 keeps M * lda * 2 below 2^31 and takes the v5 kernel's 32-bit buffer offsets,
    M = 7098 is past it and must take the 128 x 128 kernel instead.  ~2.2 GB of A on the device, only the first K columns of each row
    used (the rest NaN, so that a read outside them shows); fp64 on sampled rows, the last ones in particular."""
    K = N = 768
    lda = 197 * K
    A = torch.full((M * lda,), float("nan"), dtype=torch.float16, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(M)
    A.view(M, lda)[:, :K] = (torch.randn((M, K), generator=gen, device="cuda") * 0.5).half()
    g = torch.Generator().manual_seed(M)
    Wt = (torch.randn(N, K, generator=g) * K ** -0.5).half()
    b = (torch.randn(N, generator=g) * 0.1).half()
    rows = torch.tensor(sorted(set(_sample_rows(M, M).tolist()) | set(range(M - 520, M))))
    ref = _ref_gemm_f16(A.view(M, lda)[rows.cuda(), :K].float().cpu(), Wt, b, None, None, EPI_BIAS, 1.0, 0, 0)
    Wd, bd = Wt.cuda(), b.cuda()
    C = _sentinel(M + PAD_ROWS, N)
    for variant in GEMM_VARIANTS:
        C.view(torch.int16).fill_(SENTINEL)
        assert _gemm_strided(lib, variant, A, lda, Wd, K, bd, None, 0, C, N, M, N, K, EPI_BIAS) == 0
        torch.cuda.synchronize()
        assert _untouched(C[M:]), f"variant {variant}: wrote behind the last row"
        assert bool(torch.isfinite(C[:M]).all()), f"variant {variant}: non-finite output (read outside the K columns?)"
        _assert_gemm_close(C[rows.cuda()].float().cpu(), ref, f"variant {variant}")
    del A
    torch.cuda.empty_cache()


# ---- f. attention for the first Lq queries -----------------------------------------------------------------------------------

def _attn_kernel(variant, L, Lq):
    """The kernel launch_attention_f16_q (attention.hip) picks for a non-causal launch with L > 32."""
    if variant in (3, 4):
        if Lq == L and 192 < L <= 208:
            return "v3"
        variant = 5
    if variant == 5:
        if L >= 256 and Lq >= 32:
            return "v5"
        variant = 1
    return "v1" if variant == 1 and L >= 128 else "v0"


def _qkv_on_device(B, L, H, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    qkv = torch.randn((B * L, 3 * H * 64), generator=g, device="cuda").half()
    D = H * 64
    late = L - 70 if L >= 256 else L - 5                   # a key in the LAST key block (the lazily rescaled kernels move their max there)
    for b in {0, B - 1}:                                   # first and last sequence: spikes that only the right sequence's rows see
        qkv[b * L + L // 2, D:D + 64] *= 6.0
        qkv[b * L + late, D:D + 64] *= 9.0
    return qkv


def _ref_first_queries(qkv, seqs, L, Lq, H):
    """_ref_attention's statement for the first Lq query rows of the listed sequences: [len(seqs) * Lq, H*64] fp32."""
    n = len(seqs)
    sub = qkv.view(-1, L, 3 * H * 64)[seqs.cuda()].cpu()
    q, k, v = sub.double().reshape(n, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = q[:, :, :Lq] @ k.transpose(-1, -2) * 0.125
    return (s.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(n * Lq, H * 64).float()


def _check_attention_q(lib, B, L, Lq, H, variants):
    qkv = _qkv_on_device(B, L, H, B * L + Lq + H)
    seqs = torch.tensor(sorted({0, 1 % B, B // 2, max(0, B - 2), B - 1}))
    ref = _ref_first_queries(qkv, seqs, L, Lq, H)
    out = _sentinel(B * Lq + PAD_ROWS, H * 64)
    for variant in variants:
        what = f"variant {variant} ({_attn_kernel(variant, L, Lq)})"
        out.view(torch.int16).fill_(SENTINEL)
        assert lib.ovmr_debug_attention_q(variant, _p(qkv), _p(out), B, L, Lq, H, 0, _s()) == 0
        torch.cuda.synchronize()
        assert _untouched(out[B * Lq:]), f"{what}: wrote behind row B*Lq"
        assert bool(torch.isfinite(out[:B * Lq]).all()), f"{what}: unwritten or non-finite rows"
        got = out[:B * Lq].view(B, Lq, -1)[seqs.cuda()].float().cpu().reshape(len(seqs) * Lq, -1)
        assert float((got - ref).abs().max()) < 6e-3, f"{what}: max err {(got - ref).abs().max()}"
        kernel = _attn_kernel(variant, L, Lq)
        if kernel == _attn_kernel(variant, L, L):
            # Against the all-query launch, bit for bit.  v1 and v5 move their softmax reference on a ballot over a query tile (16 / 32
            # rows), and the spare rows of the subset launch's last tile repeat query Lq - 1 -- they must not read the Q slots behind it,
            # which the last vision block leaves unwritten (test_hip_poison.py).  So: (i) every complete tile equals the all-query
            # launch on the same qkv (v0 has no ballot: every row does); (ii) EVERY row equals the all-query launch on the qkv whose
            # Q rows from Lq on repeat row Lq - 1, where the last tile holds the same voters.
            tile = {"v0": 1, "v1": 16, "v5": 32}[kernel]
            whole = Lq // tile * tile
            rep = qkv.clone()
            rep.view(B, L, -1)[:, Lq:, :H * 64] = rep.view(B, L, -1)[:, Lq - 1:Lq, :H * 64]
            full = torch.empty((B * L, H * 64), dtype=torch.float16, device="cuda")
            for src, rows, name in ((qkv, whole, "the same qkv"), (rep, Lq, "the qkv whose Q rows from Lq on repeat row Lq - 1")):
                assert lib.ovmr_debug_attention(0, variant, _p(src), _p(full), B, L, H, 0, _s()) == 0
                torch.cuda.synchronize()
                first = full.view(B, L, -1)[:, :rows]
                assert torch.equal(out[:B * Lq].view(B, Lq, -1)[:, :rows].view(torch.int16), first.view(torch.int16)), \
                    f"{what}: != the first {rows} rows of the full launch on {name}"
            del rep, full
    assert lib.ovmr_debug_attention_q(variants[0], _p(qkv), _p(out), B, L, L + 1, H, 0, _s()) == -2


@pytest.mark.parametrize("H", [12, 16])
@pytest.mark.parametrize("B", [1, 7, 256])
@pytest.mark.parametrize("L", [50, 77, 197, 257, 577])
def test_attention_cls_query_only(lib, L, B, H):
    """Lq = 1, the last vision block's CLS query: output row b is sequence b's query 0, against fp64 on the first, middle and last
    sequences, the rows behind B stay sentinel, Lq > L is refused with -2.  Bit-equal to the first row of each sequence of the
    all-query launch wherever both take the same kernel (v0 at L < 128 and under variant 0, v1 under variants 1 / 3 / 5 for L >= 128
    where the all-query launch does not go to v3 / v5) -- for v1, whose tile votes on moving the softmax reference, of the all-query
    launch in which the tile's other rows repeat the CLS query, as the spare rows of the CLS-only launch do (_check_attention_q)."""
    _check_attention_q(lib, B, L, 1, H, ATTN_VARIANTS)


@pytest.mark.parametrize("Lq", [16, 17, 33, 64])
@pytest.mark.parametrize("L", [197, 257, 577])
def test_attention_query_subset(lib, L, Lq):
    """Lq in {16, 17, 33, 64}: ragged query tiles of v0 / v1 (16-row tiles) and v5's Lq >= 32 path (32-row tiles, 3- or 4-wave
    workgroups by the tile count).  fp64 and sentinel as above; bit-equal to the all-query launch wherever the kernel is the same --
    for v5 as well: a query tile's arithmetic does not depend on the workgroup's wave count or on the other tiles.  The ragged last
    tile of v1 / v5 is compared with the all-query launch whose rows behind Lq repeat query Lq - 1 (_check_attention_q)."""
    _check_attention_q(lib, 3, L, Lq, 12, ATTN_VARIANTS)


# ---- g. fp32 attention up to its limit ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [67, 100, 127, 128])
def test_attention_f32_up_to_its_limit(lib, L):
    """The aggregator's fp32 attention (one thread per query, K and V of the head in dynamic LDS) at L = n_ctx + shots up to 128,
    where K + V take exactly 64 KiB; 1024 (sequence, head) workgroups, several per CU.  L = 129 is refused with -2."""
    B, H = 128, 8
    g = torch.Generator().manual_seed(L)
    qkv = torch.randn(B * L, 3 * H * 64, generator=g)
    qkv[L // 2, H * 64:H * 64 + 64] *= 4.0
    qd = qkv.cuda()
    out = torch.empty(B * L + PAD_ROWS, H * 64, device="cuda")
    out.view(torch.int32).fill_(0x5A5A5A5A)
    assert lib.ovmr_debug_attention(1, 0, _p(qd), _p(out), B, L, H, 0, _s()) == 0
    torch.cuda.synchronize()
    assert bool((out[B * L:].view(torch.int32) == 0x5A5A5A5A).all())
    seqs = torch.tensor([0, 1, B // 2, B - 1])
    sub = qkv.view(B, L, -1)[seqs].reshape(len(seqs) * L, -1)
    ref = _ref_attention(sub, len(seqs), L, H, 0)
    got = out[:B * L].view(B, L, -1)[seqs.cuda()].cpu().reshape(len(seqs) * L, -1)
    torch.testing.assert_close(got, ref, atol=2e-5, rtol=1e-4)
    assert bool(torch.isfinite(out[:B * L]).all())
    big = torch.zeros(B * (L + 1), 3 * H * 64, device="cuda") if L == 128 else None
    if big is not None:
        assert lib.ovmr_debug_attention(1, 0, _p(big), _p(out), B, 129, H, 0, _s()) == -2
