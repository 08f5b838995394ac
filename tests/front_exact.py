"""The reference, the cases and the operands for the front of the image tower: the patch gather inside the patch-embedding GEMM
(GemmArgs::im2col_R, a_off / a_tile in ovmr_amd/csrc/gemm_f16_v5.hip, behind ovmr_debug_gemm_patches), the im2col pass and the CLS-row fill
(im2col_kernel, fill_cls_kernel in rowops.hip, behind ovmr_debug_im2col / ovmr_debug_fill_cls).  Plain torch, no library: shared by
test_hip_front_exact.py (GPU) and test_front_exact_cpu.py (which ties the reference to conv1 and proves that every case rejects the
index mistakes it is there for).  Nothing here is compared at a tolerance.

The reference is unfold(img, P, Kpad): row (b, gy, gx), column k = c * P * P + ky * P + kx, +0 from 3 * P * P on -- the conv weight's own
[3, P, P] order, so unfold(img) @ W.T is conv2d(img, W.view(N, 3, P, P), stride = P) (asserted in fp64).  fold is its inverse for P = 16.

The fused GEMM.  A case (B, R, N) is gemm_exact's EPI_PATCH case of M = B * G * G rows (G = R / 16), K = 768, rows_in -> rows_out = G * G ->
G * G + 1: its operands are gemm_exact.operands -- dense +-k/16, every partial sum exact in fp32 in any order -- the image is fold(A), and
the expected output is gemm_exact.expected: ONE bit pattern.  gemm_exact.route(v, M, N, 768, EPI_PATCH, im2col = R) names the kernel of
every variant (test_gemm_route_cpu.py holds that function to the library); assert_coverage requires both tile heights, the ping-pong loop
with and without groups of four N tiles, and the nontemporal stores (GUARD: 341 images of 1024 x 1024, the most whose bytes stay below
2^31; it has a test of its own).  Every variant gathers in the tile kernel: the 128 x 128 and the split-K kernels cannot.

The im2col pass.  Images carry their position: the value at (b, c, y, x) differs from that of every neighbour and of the same position in
the next image (coded_image).  The fp32 images carry, scattered over them, the values at which a cast to fp16 can go wrong (CAST_VALUES:
ties, 65519 / 65520, beyond fp16, fp16 subnormals, -0.0; no NaN); the expected matrix is unfold(img).half() on the CPU, compared as bits.

Not reached: the block cap of grid1d in launch_im2col (65535 * 16 blocks of 256 threads) needs a patch matrix of 4 GB.
"""
import functools

import torch

import gemm_exact as G

K16 = 768                                        # 3 * 16 * 16: the K of the fused GEMM
F16, F32 = 0, 1                                  # OVMR_F16, OVMR_F32 (include/ovmr_hip.h)


# ---- the reference --------------------------------------------------------------------------------------------------------------

def unfold(img, P, Kpad=None):
    """img [B, 3, R, R] -> [B * G * G, Kpad] of the same type: row (b, gy, gx), column c * P * P + ky * P + kx, +0 from 3 * P * P on."""
    B, C, R, R2 = img.shape
    assert C == 3 and R == R2 and R % P == 0
    G_, K = R // P, 3 * P * P
    Kpad = K if Kpad is None else Kpad
    out = torch.zeros((B * G_ * G_, Kpad), dtype=img.dtype)
    out[:, :K] = img.view(B, 3, G_, P, G_, P).permute(0, 2, 4, 1, 3, 5).reshape(B * G_ * G_, K)
    return out


def fold(A, R):
    """The inverse of unfold for P = 16, Kpad = 768: A [B * G * G, 768] -> [B, 3, R, R]."""
    G_ = R // 16
    B = A.shape[0] // (G_ * G_)
    assert R % 16 == 0 and A.shape == (B * G_ * G_, K16)
    return A.view(B, G_, G_, 3, 16, 16).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, R, R).contiguous()


# ---- named mutants of the reference: the index mistakes a gather can make.  Each maps (the true matrix [M, Kpad], B, G, P) to the matrix
# ---- a kernel with that mistake would read; applies(): the shapes at which the mistake is a different function at all. ------------------

def _m_kxky(A, B, G_, P):
    out = A.clone()
    out[:, :3 * P * P] = A[:, :3 * P * P].view(-1, 3, P, P).transpose(2, 3).reshape(-1, 3 * P * P)
    return out


def _m_gygx(A, B, G_, P):
    return A.view(B, G_, G_, -1).transpose(1, 2).reshape(A.shape)


def _m_channels(A, B, G_, P):
    out = A.clone()
    out[:, :3 * P * P] = A[:, :3 * P * P].view(-1, 3, P * P).flip(1).reshape(-1, 3 * P * P)
    return out


def _m_chunk(A, B, G_, P):
    return A.view(A.shape[0], -1, 8).roll(1, 1).reshape(A.shape)


def _m_last_row(A, B, G_, P):
    out = A.clone()
    out[-1] = A[-2]
    return out


def _m_neighbour(A, B, G_, P):
    out = A.clone().view(B, G_ * G_, -1)
    out[B // 2] = A.view(B, G_ * G_, -1)[B // 2 - 1 if B // 2 else 1]
    return out.view(A.shape)


def _m_padding(A, B, G_, P):
    out = A.clone()
    out[:, 3 * P * P:] = 1.0
    return out


def _m_last_column(A, B, G_, P):
    """The image's last pixel column (x = R - 1: kx = P - 1 of the patches gx = G - 1) is not read: zero."""
    out = A.clone().view(B, G_, G_, -1)
    last = out[:, :, G_ - 1, :3 * P * P].reshape(B, G_, 3, P, P).clone()
    last[..., P - 1] = 0
    out[:, :, G_ - 1, :3 * P * P] = last.reshape(B, G_, 3 * P * P)
    return out.view(A.shape)


MUTANTS = {
    "kx and ky transposed": _m_kxky,
    "gy and gx transposed": _m_gygx,
    "channels reversed": _m_channels,
    "an 8-pixel chunk shifted by one chunk": _m_chunk,
    "the last row read from row M - 2": _m_last_row,
    "one image's patches taken from its neighbour": _m_neighbour,
    "padding 1.0 instead of 0": _m_padding,
    "the last pixel column dropped": _m_last_column,
}


def applies(name, B, G_, P, Kpad):
    """False where the mutant is the SAME function as the reference at this shape, so that no operand can tell them apart: a grid of one
    patch has no gy / gx to transpose, one image has no neighbour, one row has no row M - 2, Kpad = 3 * P * P has no padding."""
    return {"gy and gx transposed": G_ >= 2, "one image's patches taken from its neighbour": B >= 2,
            "the last row read from row M - 2": B * G_ * G_ >= 2, "padding 1.0 instead of 0": Kpad > 3 * P * P}.get(name, True)


# ---- the fused GEMM: cases --------------------------------------------------------------------------------------------------------

_D128, _D256 = G._v5(128, "double"), G._v5(256, "double")
_PP, _PPG4 = G._v5(256, "pingpong"), G._v5(256, "pingpong", g4="g4")
_ALL128 = {0: _D128, 6: _D128, 8: _D128, 9: _D128}
# (B, R, N) -> variant -> the branch the case is in the list for (test_front_exact_cpu.py asserts them)
FUSED = {
    (6, 112, 136): _ALL128,                                      # M = 294: two 128-row tiles and 38 rows; ragged N tile; 49-patch images
    (65, 32, 128): _ALL128,                                      # M = 260: four patches an image
    (260, 16, 128): _ALL128,                                     # G = 1: every row another image
    (2, 224, 264): _ALL128,                                      # M = 392: the engine's 196-patch images
    (88, 112, 2048): {0: _PPG4, 6: _D256, 8: _PPG4, 9: _PPG4},     # M = 4312: ragged last 256-row tile, every tile spans five or six images
    (168, 112, 1024): {0: _PP, 6: _D256, 8: _PP, 9: _PP},           # M = 8232: four N tiles, all in one group
}
GUARD_R, GUARD_N, GUARD_B = 1024, 128, 341                     # 341 * 3 * 1024 * 1024 * 2 = 2 145 386 496 < 2^31 <= 342 * ...
GUARD_WANT = {6: G._v5(256, "double", nt="nt"), 8: G._v5(256, "pingpong", nt="nt")}
REQUIRED = (_D128, _D256, _PP, _PPG4, GUARD_WANT[6], GUARD_WANT[8])


def fused_case(B, R, N, want=None):
    """gemm_exact's Case of a fused launch: M = B * G * G patch rows, EPI_PATCH, rows_in -> rows_out = G * G -> G * G + 1."""
    g2 = (R // 16) ** 2
    return G.Case("f16", B * g2, N, K16, G.EPI_PATCH, want if want is not None else FUSED.get((B, R, N), {}), rows=(g2, g2 + 1))


def fused_route(variant, B, R, N):
    return G.route(variant, B * (R >> 4) ** 2, N, K16, G.EPI_PATCH, im2col=R)


def assert_coverage(cases=None):
    got = {fused_route(v, *k) for k in (FUSED if cases is None else cases) for v in G.GEMM_VARIANTS}
    got |= {fused_route(v, GUARD_B, GUARD_R, GUARD_N) for v in GUARD_WANT}
    missing = [b for b in REQUIRED if b not in got]
    assert not missing, f"the fused cases do not reach: {missing}"


def fused_image(c, R):
    """The fp16 images [B, 3, R, R] whose patch matrix is the case's A."""
    return fold(G.operands(c)[0], R)


# ---- the im2col pass: cases and operands --------------------------------------------------------------------------------------------

# (P, R, Kpad): both paths of the kernel -- 8 pixels at a time where P % 8 == 0, one at a time with zero padding for P = 14 (K = 588,
# Kpad = 640: the chunk 584 .. 591 straddles K) -- at one patch an image (R = P) and at grids of 2, 3 and 7
IM2COL = [(16, 16, 768), (16, 32, 768), (16, 112, 768), (14, 14, 640), (14, 42, 640), (32, 64, 3072)]
IM2COL_B = (1, 3, 17)

_T = 2.0 ** -11                                   # half an fp16 step at 1
CAST_VALUES = (
    1 + _T, 1 + 3 * _T, -(1 + _T), -(1 + 3 * _T), 1 + _T + 2.0 ** -23, 1 + _T - 2.0 ** -23,      # ties to even (down, up), and just off a tie
    2049.0, 2051.0, 65519.0, 65520.0, -65519.0, -65520.0, 65504.0,                                # the last finite value and its tie to inf
    1.0e5, -1.0e5, 2.0 ** 127, -(2.0 ** 127), float("inf"), float("-inf"),                                 # beyond fp16
    2.0 ** -24, 2.0 ** -25, -(2.0 ** -25), 2.0 ** -25 * (1 + 2.0 ** -10), 3 * 2.0 ** -25, 2.0 ** -26,   # fp16 subnormals, their ties, below them
    2.0 ** -14 - 2.0 ** -25, 1023 * 2.0 ** -24, 2.0 ** -14, -0.0, 0.0,
)


@functools.lru_cache(maxsize=4)
def coded_image(B, R):
    """fp16 [B, 3, R, R]: ((131 b + 37 c + 11 y + 3 x) mod 2039 - 1019) / 256 -- 2039 is prime and R <= 224: (b, c, y, x) and its neighbour
    in any direction, or the same position of the next image, differ."""
    b, c, y, x = torch.meshgrid(torch.arange(B), torch.arange(3), torch.arange(R), torch.arange(R), indexing="ij")
    t = ((b * 131 + c * 37 + y * 11 + x * 3) % 2039 - 1019).double() / 256
    assert torch.equal(t.half().double(), t)
    return t.half()


def cast_image(B, R):
    """fp32 [B, 3, R, R]: coded_image with CAST_VALUES written over every 5th element, in turn (5 and len(CAST_VALUES) = 30 against the
    patch widths: every value falls on many (ky, kx))."""
    img = coded_image(B, R).float().clone()
    flat = img.view(-1)
    n = (flat.numel() + 4) // 5
    vals = torch.tensor(CAST_VALUES, dtype=torch.float32)
    assert torch.equal(vals.double(), torch.tensor(CAST_VALUES, dtype=torch.float64)), "a cast value that is no fp32 value"
    flat[::5] = vals[torch.arange(n) % len(CAST_VALUES)]
    return img


def im2col_image(dtype, B, R):
    return cast_image(B, R) if dtype == F32 else coded_image(B, R)


def im2col_expected(img, P, Kpad):
    return unfold(img, P, Kpad).half()


def cls_row(W):
    """fp16 [W]: ((89 + 3 c) mod 1021 - 510) / 128, neighbouring columns distinct, none the sentinel."""
    t = ((89 + 3 * torch.arange(W)) % 1021 - 510).double() / 128
    assert torch.equal(t.half().double(), t)
    return t.half()
