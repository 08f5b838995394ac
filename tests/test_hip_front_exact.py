"""The front of the image tower held to exact values (front_exact.py: the reference, the cases and why each is in the list;
test_front_exact_cpu.py: the reference is conv1 and every case rejects the index mistakes it is there for).

  * the patch gather inside the patch-embedding GEMM (ovmr_debug_gemm_patches: the GemmArgs and the launch of ovmr_encode_image): for
    every case and every variant in {0, 6, 8, 9} rc 0 and the output equal to gemm_exact.expected bit for bit; the CLS rows and PAD_ROWS rows
    behind the output keep the sentinel; the images sit between two images of NaN, so a read outside [0, B) shows as a non-finite
    output; the same bits come from ovmr_debug_gemm on the matrix ovmr_debug_im2col wrote from the same images;
  * what the gather refuses (R % 16, N < 128, M < 256, an image pointer that is not 16-byte aligned): the rc of gemm_exact.route --
    for the pointer -2, the launcher's aligned16 test: no launch with a misaligned DMA source -- and nothing written;
  * the images' byte bound: 341 images of 1024 x 1024 (2 145 386 496 bytes, the last lane offsets just below 2^31) run under variants 6
    and 8 with exact bits on the first and the last two images; 342 are refused.  The gather's own guard stood at 2^32 and never decided
    anything: an image is rows_in * 768 * 2 bytes, so the tile kernel's test of M * lda * 2 against 2^31 (lda = 768) refuses 342 images
    first, with -4.  The guard now states 2^31 as well (gemm_f16_route, gemm_exact._route_v5; test_gemm_route_cpu.py holds the -2 it
    gives for a part-used 342nd image): no lane offset of this library reaches 2^31;
  * the im2col pass: every element of [B * G * G, Kpad], padding included, as bits, for P = 16 / 14 / 32, fp16 and fp32 images (the cast:
    front_exact.CAST_VALUES), B = 1 / 3 / 17, and an image 2 (fp32: 4) bytes into its allocation; guard rows either side keep the sentinel.
    (The block cap of grid1d in launch_im2col needs a 4 GB patch matrix and stays unreached.)
  * fill_cls: the CLS rows equal cls_pos as bits, every other row and the guard rows keep the sentinel;
  * argument errors of the three hooks launch nothing.

Needs an MI355X: run with `pytest -m gpu`.
"""
import ctypes
import time

import pytest
import torch

import front_exact as F
import gemm_exact as G
import rowops_exact as X
from conftest import usable_threads

pytestmark = pytest.mark.gpu
E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import runtime
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    torch.set_num_threads(usable_threads())
    return runtime.load_library()


def _p(t, byte_offset=0):
    return ctypes.c_void_p(t.data_ptr() + byte_offset)


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _pool(img):
    """The images on the device between two images of NaN: (pool [B + 2, 3, R, R], the view of the B images)."""
    pool = torch.full((img.shape[0] + 2,) + tuple(img.shape[1:]), float("nan"), dtype=img.dtype, device="cuda")
    pool[1:-1] = img.cuda()
    return pool, pool[1:-1]


def _intact(buf):
    return bool((G.bits(buf) == (G.SENTINEL32 if buf.dtype == torch.float32 else G.SENTINEL)).all())


# ---- the fused gather ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", list(F.FUSED), ids=str)
def test_patch_gather_exact(lib, key):
    t0 = time.time()
    B, R, N = key
    c = F.fused_case(*key)
    ops = G.operands(c)
    A, W, _, _, pos = ops
    want, _ = G.expected(c, ops)
    want = want.cuda()
    G.bits(want)[~G.compared_rows(c).cuda()] = G.SENTINEL                   # the CLS rows must keep the sentinel
    pool, img = _pool(F.fused_image(c, R))
    Wd, pd = W.cuda(), pos.cuda()
    # the im2col pass on the same images gives A itself
    colbuf, col = X.guarded(c.M, F.K16, device="cuda")
    assert lib.ovmr_debug_im2col(_p(img), F.F16, B, R, 16, F.K16, _p(col), _s()) == 0
    torch.cuda.synchronize()
    msg = G.bits_mismatch(col, A.cuda())
    assert msg is None and X.guards_untouched(colbuf, c.M) is None, f"{key}: im2col: {msg}"
    for variant in G.GEMM_VARIANTS:
        what = f"{key}, variant {variant}: {F.fused_route(variant, *key)}"
        buf = G.sentinel_buffer(c.out_rows + G.PAD_ROWS, N, device="cuda")
        rc = lib.ovmr_debug_gemm_patches(variant, _p(img), R, _p(Wd), _p(pd), _p(buf), B, N, _s())
        assert rc == 0, f"{what}: rc {rc}"
        torch.cuda.synchronize()
        msg = G.outside_untouched(buf, c.out_rows, N)
        assert msg is None, f"{what}: {msg}"
        assert bool(torch.isfinite(buf).all()), f"{what}: non-finite output: read outside the B images"
        msg = G.bits_mismatch(buf[:c.out_rows], want)
        assert msg is None, f"{what}: {msg}"
        two = G.sentinel_buffer(c.out_rows + G.PAD_ROWS, N, device="cuda")
        rc = lib.ovmr_debug_gemm(0, variant, _p(col), _p(Wd), None, None, _p(pd), _p(two), c.M, N, F.K16, N, G.EPI_PATCH, 1.0, c.rows[0], c.rows[1], _s())
        assert rc == 0, f"{what}: the GEMM on the im2col matrix: rc {rc}"
        torch.cuda.synchronize()
        msg = G.bits_mismatch(two, buf)
        assert msg is None, f"{what}: against the GEMM on the im2col matrix: {msg}"
    print(f"\n{key}: {time.time() - t0:.2f} s")


# (B, R, N, byte offset of the image pointer): what the gather refuses
REFUSED = [(300, 24, 128, 0), (6, 112, 120, 0), (5, 112, 128, 0), (6, 112, 136, 2), (6, 112, 136, 8), (88, 112, 2048, 2)]


@pytest.mark.parametrize("B,R,N,off", REFUSED, ids=str)
def test_patch_gather_refusals_write_nothing(lib, B, R, N, off):
    g2 = (R >> 4) ** 2
    img = torch.full((B + 1, 3, R, R), 0.5, dtype=torch.float16, device="cuda")
    Wd = torch.full((N, F.K16), 0.25, dtype=torch.float16, device="cuda")
    pd = torch.ones((g2 + 1, N), dtype=torch.float16, device="cuda")
    for variant in G.GEMM_VARIANTS:
        # a pointer that is not 16-byte aligned: the route (stated for aligned operands) names a kernel, the launcher's aligned16 test is -2
        want = ("err", -2) if off else F.fused_route(variant, B, R, N)
        assert want[0] == "err" and want[1] != 0, f"({B}, {R}, {N}) is no refusal under variant {variant}: {want}"
        buf = G.sentinel_buffer(B * (g2 + 1) + G.PAD_ROWS, N, device="cuda")
        rc = lib.ovmr_debug_gemm_patches(variant, _p(img, off), R, _p(Wd), _p(pd), _p(buf), B, N, _s())
        torch.cuda.synchronize()
        assert rc == want[1], f"variant {variant}: rc {rc}, the route states {want[1]}"
        assert _intact(buf), f"variant {variant}: a refused launch wrote"


def _signed16_cuda(shape, gen):
    """+-k/16, 1 <= k <= 15, on the device (gemm_exact._signed)."""
    r = torch.randint(0, 30, shape, generator=gen, device="cuda", dtype=torch.int16)
    return (r - 15 + (r >= 15).to(torch.int16)).half() / 16


def test_patch_gather_at_the_image_byte_bound(lib):
    """See the module docstring.  2.2 GB of images on the device, filled there; the reference is computed on the CPU from images 0, 339
    and 340 alone.  The allocations are freed at the end."""
    t0 = time.time()
    B, R, N = F.GUARD_B, F.GUARD_R, F.GUARD_N
    g2 = (R // 16) ** 2
    L = g2 + 1
    assert B * 3 * R * R * 2 < 2 ** 31 - 1 <= (B + 1) * 3 * R * R * 2
    pool = torch.empty((B + 2, 3, R, R), dtype=torch.float16, device="cuda")      # [0] and [B + 1]: NaN
    pool[0] = float("nan")
    pool[-1] = float("nan")
    gen = torch.Generator(device="cuda").manual_seed(B)
    for b in range(1, B + 1, 31):
        pool[b:min(b + 31, B + 1)] = _signed16_cuda((min(b + 31, B + 1) - b, 3, R, R), gen)
    img = pool[1:]
    picked = [0, B - 2, B - 1]
    c3 = F.fused_case(len(picked), R, N, {})
    _, W, bias, res, pos = G.operands(c3)
    A3 = F.unfold(img[picked].cpu(), 16)
    G.assert_exact(A3, W, "the picked images")
    want3 = G.epilogue(c3, G.product(A3, W), bias, res, pos).view(len(picked), L, N)[:, 1:].cuda()
    Wd, pd = W.cuda(), pos.cuda()
    rows = B * L
    buf = G.sentinel_buffer(rows + L + G.PAD_ROWS, N, device="cuda")              # room for a 342nd image, should a refused launch run
    for variant in (6, 8):
        what = f"variant {variant}: {F.fused_route(variant, B, R, N)}"
        assert F.fused_route(variant, B, R, N) == F.GUARD_WANT[variant]
        G.bits(buf).fill_(G.SENTINEL)
        t1 = time.time()
        rc = lib.ovmr_debug_gemm_patches(variant, _p(img), R, _p(Wd), _p(pd), _p(buf), B, N, _s())
        assert rc == 0, f"{what}: rc {rc}"
        torch.cuda.synchronize()
        t1 = time.time() - t1
        assert _intact(buf[rows:]), f"{what}: wrote behind the last row"
        out = buf[:rows].view(B, L, N)
        assert _intact(out[:, 0]), f"{what}: wrote a CLS row"
        assert bool(torch.isfinite(out).all()), f"{what}: non-finite output: read outside the B images"
        for i, b in enumerate(picked):
            msg = G.bits_mismatch(out[b, 1:], want3[i])
            assert msg is None, f"{what}: image {b}: {msg}"
        print(f"\n{what}: launch {t1:.2f} s")
        # one image more: refused, nothing written
        want = F.fused_route(variant, B + 1, R, N)
        assert want == ("err", -4)
        G.bits(buf).fill_(G.SENTINEL)
        rc = lib.ovmr_debug_gemm_patches(variant, _p(pool), R, _p(Wd), _p(pd), _p(buf), B + 1, N, _s())
        torch.cuda.synchronize()
        assert rc == want[1] and _intact(buf), f"{what}: {B + 1} images: rc {rc}"
    del pool, img, buf, out
    torch.cuda.empty_cache()
    print(f"\nthe image byte bound: {time.time() - t0:.2f} s")


# ---- the im2col pass ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", F.IM2COL, ids=str)
def test_im2col_exact(lib, case):
    P, R, Kpad = case
    g2 = (R // P) ** 2
    for dtype in (F.F16, F.F32):
        item = 4 if dtype == F.F32 else 2
        for B in F.IM2COL_B:
            img = F.im2col_image(dtype, B, R)
            want = F.im2col_expected(img, P, Kpad).cuda()
            for shift in (0, 1):                                        # the image one element into its allocation: the pass loads elements
                store = torch.full((img.numel() + 8,), float("nan"), dtype=img.dtype, device="cuda")
                store[shift:shift + img.numel()] = img.reshape(-1).cuda()
                buf, out = X.guarded(B * g2, Kpad, device="cuda")
                rc = lib.ovmr_debug_im2col(_p(store, shift * item), dtype, B, R, P, Kpad, _p(out), _s())
                torch.cuda.synchronize()
                what = f"{case}, {'fp32' if dtype else 'fp16'}, B = {B}, image {shift * item} bytes into its allocation"
                assert rc == 0, f"{what}: rc {rc}"
                assert X.guards_untouched(buf, B * g2) is None, f"{what}: {X.guards_untouched(buf, B * g2)}"
                msg = G.bits_mismatch(out, want)
                assert msg is None, f"{what} (column = c * {P * P} + ky * {P} + kx, padding from {3 * P * P}): {msg}"


# ---- fill_cls -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [128, 768, 1024])
def test_fill_cls_exact(lib, W):
    cls = F.cls_row(W)
    cd = cls.cuda()
    for L in (2, 50):
        for B in (1, 3, 257):
            buf, x = X.guarded(B * L, W, device="cuda")
            rc = lib.ovmr_debug_fill_cls(_p(x), _p(cd), B, L, W, _s())
            torch.cuda.synchronize()
            what = f"W = {W}, L = {L}, B = {B}"
            assert rc == 0, f"{what}: rc {rc}"
            assert X.guards_untouched(buf, B * L) is None, f"{what}: {X.guards_untouched(buf, B * L)}"
            rows = x.view(B, L, W)
            assert torch.equal(G.bits(rows[:, 0]), G.bits(cd).expand(B, W)), f"{what}: a CLS row is not cls_pos"
            assert _intact(rows[:, 1:]), f"{what}: wrote a row that is no CLS row"


# ---- argument errors ------------------------------------------------------------------------------------------------------------

def test_front_hooks_argument_errors_launch_nothing(lib):
    z = None
    img = torch.zeros((2, 3, 32, 32), dtype=torch.float16, device="cuda")
    w = torch.zeros((128, F.K16), dtype=torch.float16, device="cuda")
    out = G.sentinel_buffer(2 * 5 + 64, F.K16, device="cuda")
    i, o, wp, s = _p(img), _p(out), _p(w), _s()
    calls = [
        lambda: lib.ovmr_debug_im2col(z, F.F16, 2, 32, 16, 768, o, s), lambda: lib.ovmr_debug_im2col(i, F.F16, 2, 32, 16, 768, z, s),
        lambda: lib.ovmr_debug_im2col(i, F.F16, -1, 32, 16, 768, o, s), lambda: lib.ovmr_debug_im2col(i, 2, 2, 32, 16, 768, o, s),
        lambda: lib.ovmr_debug_im2col(i, F.F16, 2, 32, 0, 768, o, s), lambda: lib.ovmr_debug_im2col(i, F.F16, 2, 32, 12, 768, o, s),
        lambda: lib.ovmr_debug_im2col(i, F.F16, 2, 32, 16, 760, o, s), lambda: lib.ovmr_debug_im2col(i, F.F16, 2, 32, 16, 772, o, s),
        lambda: lib.ovmr_debug_im2col(i, F.F16, 2, -32, 16, 768, o, s),
        lambda: lib.ovmr_debug_fill_cls(z, wp, 2, 5, 768, s), lambda: lib.ovmr_debug_fill_cls(o, z, 2, 5, 768, s),
        lambda: lib.ovmr_debug_fill_cls(o, wp, -1, 5, 768, s), lambda: lib.ovmr_debug_fill_cls(o, wp, 2, 0, 768, s),
        lambda: lib.ovmr_debug_fill_cls(o, wp, 2, 5, 766, s), lambda: lib.ovmr_debug_fill_cls(o, wp, 2, 5, -4, s),
        lambda: lib.ovmr_debug_gemm_patches(8, z, 32, wp, wp, o, 2, 128, s), lambda: lib.ovmr_debug_gemm_patches(8, i, 32, z, wp, o, 2, 128, s),
        lambda: lib.ovmr_debug_gemm_patches(8, i, 32, wp, z, o, 2, 128, s), lambda: lib.ovmr_debug_gemm_patches(8, i, 32, wp, wp, z, 2, 128, s),
        lambda: lib.ovmr_debug_gemm_patches(8, i, 32, wp, wp, o, -1, 128, s), lambda: lib.ovmr_debug_gemm_patches(8, i, 32, wp, wp, o, 2, -128, s),
        lambda: lib.ovmr_debug_gemm_patches(8, i, -32, wp, wp, o, 2, 128, s),
    ]
    for n, call in enumerate(calls):
        assert call() == E_ARG, f"call {n}"
    torch.cuda.synchronize()
    assert _intact(out)
    # empty batches are no error and write nothing
    assert lib.ovmr_debug_im2col(i, F.F16, 0, 32, 16, 768, o, s) == 0 and lib.ovmr_debug_fill_cls(o, wp, 0, 5, 768, s) == 0
    assert lib.ovmr_debug_gemm_patches(8, i, 32, wp, wp, o, 0, 128, s) == 0
    torch.cuda.synchronize()
    assert _intact(out)
