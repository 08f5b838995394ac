"""Exact-operand cases and the comparator for the classifier head (ovmr_amd/csrc/head_fused.hip and the five-launch path behind
ovmr_fused_logits / ovmr_zeroshot_logits / ovmr_xval_counts).  Plain torch, no library: shared by test_hip_head_exact.py (GPU) and
test_head_exact_cpu.py (which proves that the comparator rejects the defects it is there for).

The method.  Features and classifier rows are sparse with dyadic entries, so that sf = h(scale * f) has few mantissa bits and every
product sf[b,k] * clf[c,k] is a multiple of 2^-p with sum_k |product| < 2^(24 - p).  Then every partial sum of every dot product,
in any order and grouping, is exact in fp32 (and in the MFMA's fp32 accumulator): the fp16 logit is ONE number whatever the kernel's K
order, known bit for bit.  What remains inexact in a probability is fp32 exp / reciprocal / sums:

    rtol = 1e-4, derived: the product x * log2(e) in front of v_exp_f32 carries a relative error of |x| * 2^-24 .. 2^-23 into the
    exponential, where only |x| <= 88 matters (5e-6 .. 1e-5; beyond that the term is below the fp32 normal range), the exponential and
    the reciprocal are good to 1 ulp (1.2e-7 each), the merges of (maximum, sum) pairs multiply by one more exponential, and fp32 sums
    of at most 21 841 positive terms add a few 1e-6 in the worst order: about 2e-5 in all.
    tiny = 2^-126 * (sum_m |w[c,m]| at most): an exponential below the fp32 normal range may be flushed or lose bits, before or after
    it is multiplied by 1 / sum <= 1 and by w.
"""
import math

import torch

RTOL = 1e-4
TINY = 2.0 ** -126
HF_BN = 128                                     # classes per tile of the one-launch head
MODE_CLF = {"multimodal": 0, "vision": 1, "text": 2}      # ovmr_fused_logits: which classifier a single-classifier mode reads
MODES = ("fusion", "text", "vision", "multimodal")

# (B, C, D) of every case.  D: the embedding widths of the models in synth.SPECS (tiny 128, small 256, ViT-B/16 512, head768 768).
_SMALL_B = (1, 31, 32, 33, 63, 64, 65, 255, 256)
_SMALL_C = (1, 5, 31, 33, 127, 128, 129, 1000, 1003)
_WIDTHS = (128, 256, 512, 768)
SHAPES = [(B, C, _WIDTHS[(i + j) % 4]) for i, B in enumerate(_SMALL_B) for j, C in enumerate(_SMALL_C)] + [
    (40, 2048, 128), (256, 2048, 512), (40, 2049, 256), (256, 2049, 768),        # 16 / 17 class tiles: the last local merge, the first duty phase
    (40, 2500, 512), (256, 2500, 128), (40, 10000, 768), (256, 10000, 256), (40, 21841, 768), (256, 21841, 512),
    (257, 2048, 256), (300, 2048, 128), (512, 2048, 768),                        # the entry rule's second arm (<= 512 rows x 2048 classes)
    (513, 1000, 512), (300, 4500, 256),                                          # the rule says five launches; fused_head = 2 must still be right
    (520, 2048, 256), (1100, 1003, 128),                                         # 64-row tiles with the local merge (more than 256 32-row tiles, <= 16 class tiles)
    (1540, 21841, 128),                                                          # B * C > 32 Mi logits: the five-launch path runs it in two row chunks
]


def lowbit_exponent(x):
    """Smallest p >= 0 such that every element of x is a multiple of 2^-p (x: fp16, or fp32 holding values with <= 24 fractional bits)."""
    v = x.double().abs() * 2.0 ** 24
    v = v[v != 0]
    if v.numel() == 0:
        return 0
    vi = v.to(torch.int64)
    assert bool((vi.double() == v).all()), "value with more than 24 fractional bits"
    low = int((vi & -vi).min())                              # the lowest set bit over all elements
    return max(0, 24 - (low.bit_length() - 1))


def scaled_features(feats, scale):
    """h(scale * f) as every head implementation computes it: one fp32 multiply by the handle's logit scale, one rounding to fp16."""
    return (feats.float() * torch.tensor(scale, dtype=torch.float32)).half()


def assert_exact(a, b, what):
    """The exactness condition for the products a[i,k] * b[j,k]: with p = p_a + p_b (every product is a multiple of 2^-p),
    sum_k |a[i,k] b[j,k]| <= max_i sum_k |a[i,k]| * max |b| < 2^(24 - p).  Sufficient for every partial sum to be exact in fp32."""
    p = lowbit_exponent(a) + lowbit_exponent(b)
    bound = float(a.double().abs().sum(1).max()) * float(b.double().abs().max()) if a.numel() and b.numel() else 0.0
    assert bound < 2.0 ** (24 - p), f"{what}: sum of |products| up to {bound} with p = {p}: not exact in fp32"
    return p, bound


def _sparse(g, rows, D, n, denom, kmax, kmin=1):
    """[rows, D] fp32, n non-zeros per row in the first D - 1 columns (the last one is reserved), values +-k / denom, kmin <= k <= kmax."""
    idx = torch.rand((rows, D - 1), generator=g).argsort(1)[:, :n]
    k = torch.randint(kmin, kmax + 1, (rows, n), generator=g) * (torch.randint(0, 2, (rows, n), generator=g) * 2 - 1)
    return torch.zeros((rows, D)).scatter_(1, idx, k.float() / denom)


def planted(C, n_mod):
    """(tie pairs (lo, hi): classifier row hi is a copy of row lo; the class whose row is zero in the LAST classifier, or None)."""
    Tc = (C + HF_BN - 1) // HF_BN
    ties = []
    if C >= 5:
        ties.append((1, 2))                                  # inside one wave's 32-class slice
    if C >= 72:
        ties.append((6, 70))                                 # waves 0 and 2 of class tile 0
    if C >= 139:
        ties.append((9, 137))                                # class tiles 0 and 1
    if Tc >= 3 and (Tc - 1) * HF_BN + 2 < C - 1:
        ties.append((20, (Tc - 1) * HF_BN + 2))              # the first and the last class tile
    used = {c for t in ties for c in t} | {C - 1}
    zero = next((c for c in range(C // 2, C - 1) if c not in used), None) if n_mod >= 2 and C >= 5 else None
    return ties, zero


def exact_head_case(B, C, D, n_mod, scale, seed):
    """fp16 feats [B, D], n_mod fp16 classifiers [C, D], fp32 w [C, 3] and the expected fp16 logits (one [B, C] per classifier), for
    which the exactness condition above holds (asserted).  Planted, as far as B and C have room:
      * rows b % 8 == 0 aligned with class C - 1: the row maximum sits on the last class, the one the kernel's padding lanes copy
        (rows 8, 24, ..: strongly, one dominant class and exponent arguments below -100);
      * rows 1, 5, 9, ...: all-zero features; aligned with the lower class of every tie pair (classifier row hi = row lo in every
        classifier: exact ties of the row maximum inside a wave slice, across waves, across class tiles -- the lowest column must win);
        a row that only touches the reserved last column, where every classifier row holds 1/4: all logits equal (9.375);
      * rows b % 8 == 4 aligned with two classes at once (a flat top), every other row random (spread of a few tens);
      * a zero row in the last classifier (there the all-equal row has one 0 among its 9.375s);
      * w[c, m] = 0.1 + ((5 c + 11 m) mod 17) / 17: neighbouring classes and classifiers differ by at least 5/17."""
    assert D % 64 == 0 and 1 <= n_mod <= 3 and B >= 1 and C >= 1
    g = torch.Generator().manual_seed(seed)
    wide = D > 256
    base = _sparse(g, C, D, 12 if wide else 8, 16, 4)                       # +-(1..4)/16, shared by the classifiers (they are correlated)
    clfs = []
    for m in range(n_mod):
        extra = _sparse(g, C, D, 6 if wide else 4, 16, 3)                   # +-(1..3)/16 of its own
        clfs.append(torch.where(base != 0, base, extra))
    ties, zero = planted(C, n_mod)

    def aligned(classes, kmin=2, kmax=3):
        """Features on the supports of the given classes' shared pattern, signs matched, +-(kmin..kmax)/8; a few random entries elsewhere."""
        f = _sparse(g, 1, D, 8, 8, 2)[0]
        for i, c in enumerate(classes):
            sup = (base[c] != 0).nonzero().flatten()
            sup = sup[i::len(classes)]                                      # two classes: half of each support
            mag = torch.randint(kmin, kmax + 1, (sup.numel(),), generator=g).float() / 8
            f[sup] = torch.sign(base[c][sup]) * mag
        return f

    feats = _sparse(g, B, D, 24 if wide else 16, 8, 3)                      # +-(1..3)/8: scale * f = 12.5, 25, 37.5 (exact in fp16)
    plants = [torch.zeros(D)] + [None] * len(ties) + [torch.zeros(D)]
    plants[-1][D - 1] = 3.0 / 8
    for b in range(B):
        if b % 8 == 0:
            feats[b] = aligned([C - 1], 4, 6) if b % 16 else aligned([C - 1])
        elif b % 4 == 1 and b // 4 < len(plants):
            i = b // 4
            feats[b] = plants[i] if plants[i] is not None else aligned([ties[i - 1][0]], 4, 6)
        elif b % 8 == 4 and C >= 3:
            feats[b] = aligned(torch.randint(0, C, (2,), generator=g).tolist())
    for m in range(n_mod):
        clfs[m][:, D - 1] = 0.25
        for lo, hi in ties:
            clfs[m][hi] = clfs[m][lo]
    if zero is not None:
        clfs[n_mod - 1][zero] = 0.0
    feats, clfs = feats.half(), [c.half() for c in clfs]
    assert bool((feats.abs() <= 1).all()) and all(bool((c.abs() <= 1).all()) for c in clfs)
    sf = scaled_features(feats, scale)
    logits = []
    for m in range(n_mod):
        assert_exact(sf, clfs[m], f"B={B} C={C} D={D} classifier {m}")
        logits.append((sf.double() @ clfs[m].double().t()).half())          # exact in fp64 a fortiori; ONE rounding, to fp16
    c = torch.arange(C)
    w = torch.stack([0.1 + ((5 * c + 11 * m) % 17).float() / 17 for m in range(3)], 1).contiguous()
    return feats, clfs, w, logits


def xval_expected(feats, clf, scale):
    """The cross-validation logits h(h(f . clf) * scale) (EPI_SCALE / EPI_SCALE_ARGMAX: the scale follows the product).  f . clf is exact
    under the same condition (asserted), the two roundings and the fp32 multiply are the kernel's."""
    assert_exact(feats, clf, "cross-validation product")
    dot = (feats.double() @ clf.double().t()).half()
    return (dot.float() * torch.tensor(scale, dtype=torch.float32)).half()


def xval_labels(logits16):
    """Labels for the counts: the predicted class for two rows of three, its neighbour for the third (true positives and misses)."""
    pred = first_argmax(logits16)
    b = torch.arange(pred.numel(), device=pred.device)
    return torch.where(b % 3 == 0, (pred + 1) % logits16.shape[1], pred).to(torch.int32)


# ---- the comparator ---------------------------------------------------------------------------------------------------------

def softmax64(l16):
    x = l16.double()
    e = (x - x.max(1, keepdim=True).values).exp()
    return e / e.sum(1, keepdim=True)


def reference_probs(logits, w, mode):
    """fp64 statement of ovmr_fused_logits on the expected fp16 logits: out[b,c] = sum_m w[c,m] softmax_c(l_m[b])[c], or one softmax."""
    if mode == "fusion":
        return sum(softmax64(logits[m]) * w[:, m].double() for m in range(3))
    return softmax64(logits[MODE_CLF[mode]])


def tiny_for(w, mode):
    return TINY * (max(1.0, float(w.double().abs().sum(1).max())) if mode == "fusion" else 1.0)


def _first(bad):
    return tuple(int(i) for i in bad.nonzero()[0])


def logits_mismatch(got16, want16):
    """None if the fp16 tensors are bit-equal, else the first differing (row, column) with both bit patterns."""
    g, w = got16.view(torch.int16), want16.view(torch.int16)
    if g.shape == w.shape and torch.equal(g, w):
        return None
    if g.shape != w.shape:
        return f"shape {tuple(g.shape)} != {tuple(w.shape)}"
    r, c = _first(g != w)
    return (f"{int((g != w).sum())} logits differ, first at ({r}, {c}): expected {float(want16[r, c])} (0x{int(w[r, c]) & 0xffff:04x}), "
            f"got {float(got16[r, c])} (0x{int(g[r, c]) & 0xffff:04x})")


def max_rel_error(got, ref, tiny):
    """Largest (|got - ref| - tiny)+ / ref: the figure RTOL bounds."""
    if ref.numel() == 0:
        return 0.0
    return float((((got.double() - ref).abs() - tiny).clamp(min=0) / ref).max())


def probs_mismatch(got, ref, tiny, rtol=RTOL):
    """None if |got - ref| <= rtol * ref + tiny everywhere (NaN fails), else the first offending (row, column)."""
    bad = ~((got.double() - ref).abs() <= rtol * ref + tiny)
    if not bool(bad.any()):
        return None
    r, c = _first(bad)
    return (f"{int(bad.sum())} probabilities beyond rtol {rtol:g}, first at ({r}, {c}): expected {float(ref[r, c]):.9e}, got {float(got[r, c]):.9e}; "
            f"largest relative error {max_rel_error(got, ref, tiny):.3e}")


def rowsum_mismatch(got, ref, rtol=RTOL):
    """Row sums (fp64 sum of the output) against the reference's: 1 for a single classifier, sum_c sum_m w[c,m] p_m[b,c] for the fusion."""
    s, r = got.double().sum(1), ref.sum(1)
    bad = ~((s - r).abs() <= rtol * r)
    if not bool(bad.any()):
        return None
    b = _first(bad)[0]
    return f"{int(bad.sum())} row sums beyond rtol {rtol:g}, first row {b}: expected {float(r[b]):.9e}, got {float(s[b]):.9e}"


def first_argmax(l16):
    """Row argmax with ties to the LOWEST column (torch.argmax on the CPU, the reference's rule), spelled out."""
    x = l16.float()
    C = x.shape[1]
    cols = torch.arange(C, device=x.device).expand_as(x)
    return torch.where(x == x.max(1, keepdim=True).values, cols, torch.full_like(cols, C)).min(1).values


def expected_counts(l16, labels):
    """(tp, n_pred) of trainers/mm_classifier_one_prompt.py:266-270: bincounts of the first-index argmax."""
    C = l16.shape[1]
    pred = first_argmax(l16)
    hit = pred == labels.to(pred.dtype)
    return torch.bincount(pred[hit], minlength=C).to(torch.int32), torch.bincount(pred, minlength=C).to(torch.int32)


def counts_mismatch(tp, n_pred, l16, labels):
    wtp, wnp = expected_counts(l16, labels)
    for name, got, want in (("tp", tp, wtp), ("n_pred", n_pred, wnp)):
        if not torch.equal(got.to(torch.int32), want):
            c = _first(got.to(torch.int32) != want)[0]
            return f"{name} differs in {int((got.to(torch.int32) != want).sum())} classes, first class {c}: expected {int(want[c])}, got {int(got[c])}"
    return None


# ---- which kernel instantiation a case runs (launch_head_fused's rule) ------------------------------------------------------------

def tile_rows(B, C, D, n_cu):
    """Query rows per tile: 32 while there is at most one 32-row tile per CU, else 64 (if the staged features fit 160 KiB of LDS)."""
    Tc = (C + HF_BN - 1) // HF_BN
    bm = 32 if ((B + 31) // 32) * Tc <= n_cu else 64
    if bm * (D + 8) * 2 + 4 * 3 * bm * 2 * 4 > 160 * 1024:
        bm = 32
    return bm


def head_plan(B, C):
    """The entry rule of ovmr_fused_logits at fused_head = 1: one launch up to 256 rows, or up to 512 rows x 2048 classes."""
    return B <= 256 or (B <= 512 and C <= 2048)


def coverage(shapes, n_cu):
    """What the shape list runs on a device with n_cu compute units: {(tile rows, merge form)} for the softmax kernel at its full grid,
    the same for capped grids (a cap below the tile count), and the tile heights of the raw (zero-shot) kernel."""
    soft, capped, raw = set(), set(), set()
    for B, C, D in shapes:
        Tc = (C + HF_BN - 1) // HF_BN
        bm = tile_rows(B, C, D, n_cu)
        merge = "duty" if Tc > 16 else "local"
        soft.add((bm, merge))
        raw.add(bm)
        if ((B + bm - 1) // bm) * Tc > 1:                     # head_max_grid = 1 is below the tile count
            capped.add((bm, merge))
    return soft, capped, raw


def assert_coverage(shapes, n_cu):
    soft, capped, raw = coverage(shapes, n_cu)
    missing = [f"softmax {k}" for k in ((32, "local"), (32, "duty"), (64, "local"), (64, "duty")) if k not in soft]
    missing += [f"capped grid {k}" for k in ((32, "local"), (32, "duty"), (64, "local"), (64, "duty")) if k not in capped]
    missing += [f"raw, {bm}-row tiles" for bm in (32, 64) if bm not in raw]
    assert not missing, f"the shape list does not reach, on {n_cu} CUs: {', '.join(missing)}"


# ---- a model of the one-launch head in fp64, with the defects the comparator must reject ----------------------------------------------

def simulate(logits, w, mode, defect=None, m_bad=0, t_bad=0):
    """ovmr_fused_logits the way head_fused.hip computes it -- (maximum, sum of exponentials) per 128-class tile, merged, then the weighted
    probabilities -- in fp64, optionally with ONE defect:
      "denominator": every sum of exponentials 0.1 % too large;      "drop_tile": tile t_bad's sum left out of classifier m_bad's merge;
      "unmasked_pad": the padding lanes of the last tile (copies of class C - 1) counted in its sum;
      "w_class" / "w_clf": for one class per tile (offset 77, or the last class) the weights of the neighbouring class / classifier."""
    ms = (0, 1, 2) if mode == "fusion" else (MODE_CLF[mode],)
    B, C = logits[ms[0]].shape
    Tc = (C + HF_BN - 1) // HF_BN
    wd = w.double().clone()
    if defect in ("w_class", "w_clf"):
        for t in range(Tc):
            c = min(t * HF_BN + 77, C - 1)
            wd[c] = w[c + 1 if c + 1 < C else c - 1].double() if defect == "w_class" else w[c].double().roll(1)
    out = torch.zeros((B, C), dtype=torch.float64)
    for i, m in enumerate(ms):
        x = logits[m].double()
        fill = x[:, C - 1:C].expand(B, Tc * HF_BN - C) if defect == "unmasked_pad" else torch.full((B, Tc * HF_BN - C), -math.inf, dtype=torch.float64)
        xt = torch.cat([x, fill], 1).view(B, Tc, HF_BN)
        Mt = xt.max(2).values
        St = (xt - Mt[:, :, None]).exp().sum(2)
        M = Mt.max(1).values
        part = St * (Mt - M[:, None]).exp()
        if defect == "drop_tile" and i == m_bad:
            part[:, t_bad] = 0.0
        S = part.sum(1)
        if defect == "denominator":
            S = S * 1.001
        p = (x - M[:, None]).exp() / S[:, None]
        out += p * wd[:, m] if mode == "fusion" else p
    return out


def tile_share(l16):
    """[B, Tc]: the share of a row's sum of exponentials that each 128-class tile holds."""
    B, C = l16.shape
    Tc = (C + HF_BN - 1) // HF_BN
    p = torch.cat([softmax64(l16), torch.zeros((B, Tc * HF_BN - C), dtype=torch.float64)], 1)
    return p.view(B, Tc, HF_BN).sum(2)


def step_fp16(l16, r, c):
    """A copy of l16 with element (r, c) moved to the neighbouring fp16 value (one step away from zero)."""
    out = l16.clone()
    out.view(torch.int16)[r, c] += 1
    return out
