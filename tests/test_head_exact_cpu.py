"""CPU companion of test_hip_head_exact.py: the exact-operand generator keeps its promise on every listed shape, and the comparator the
GPU test applies to the head's output rejects the defects it is there for (head_exact.simulate: an fp64 model of head_fused.hip with one
defect injected).  Pure torch: no library, no GPU.

A defect "applies" to a shape when the shape has the structure it needs (two class tiles, a ragged last tile, a tied row maximum ...).
Whether the INPUTS make it visible is asserted, not assumed: the generator plants rows with all logits equal, so from 8 rows on every class
tile holds 128 / C of some row's mass and every class a probability far above `tiny`."""
import math

import pytest
import torch

import head_exact as H

SCALES = (100.0, float(torch.tensor(math.log(100.0), dtype=torch.float32).exp()))   # exp(fp32 ln 100) = 100.00001: what the engine reports
MAX_ROWS = 48                                                 # rows on which the slow statements (sequential sums, the fp64 model) run


def _ids(s):
    return "x".join(str(v) for v in s)


def _case(shape, seed=0):
    B, C, D = shape
    scale = SCALES[(B + C) % 2]
    return scale, H.exact_head_case(B, C, D, 3, scale, 1000 * seed + B + C)


def _rows(B):
    """The planted rows (the first 32) and the last ones."""
    return torch.tensor(sorted(set(range(min(B, 32))) | set(range(max(0, B - (MAX_ROWS - 32)), B))))


@pytest.mark.parametrize("shape", H.SHAPES, ids=_ids)
def test_generator_is_exact(shape):
    """The exactness condition holds (asserted inside the generator); the expected logits equal an fp64 evaluation rounded to fp16; fp32
    sums in four different orders -- forward, reversed, blocked by 16 and by 64 -- are bit-equal to the fp64 sum."""
    B, C, D = shape
    scale, (feats, clfs, w, logits) = _case(shape)
    assert feats.dtype == torch.float16 and feats.shape == (B, D) and w.shape == (C, 3) and w.dtype == torch.float32
    sf = H.scaled_features(feats, scale)
    rows = _rows(B)
    for m in range(3):
        assert clfs[m].shape == (C, D) and logits[m].shape == (B, C) and logits[m].dtype == torch.float16
        p, bound = H.assert_exact(sf, clfs[m], "condition")
        assert p <= 8 and bound < 2 ** 16                                # far inside the limit, not at its edge
        a, b = sf[rows].float(), clfs[m].float()
        exact = a.double() @ b.double().t()
        assert torch.equal(exact.half().view(torch.int16), logits[m][rows].view(torch.int16))
        fwd = torch.zeros((rows.numel(), C))
        rev = torch.zeros((rows.numel(), C))
        for k in range(D):                                                # strictly sequential fp32 sums, one product at a time
            fwd += a[:, k, None] * b[None, :, k]
            rev += a[:, D - 1 - k, None] * b[None, :, D - 1 - k]
        assert torch.equal(fwd.double(), exact) and torch.equal(rev.double(), exact)
        for blk in (16, 64):                                              # partial sums per block, then the blocks: the MFMA's grouping
            parts = torch.einsum("bgk,cgk->gbc", a.view(-1, D // blk, blk), b.view(C, D // blk, blk))
            acc = torch.zeros((rows.numel(), C))
            for gi in range(D // blk):
                acc += parts[gi]
            assert torch.equal(acc.double(), exact)
    # the cross-validation statement, h(h(f . clf) * scale): exact product, deterministic roundings
    xv = H.xval_expected(feats[rows], clfs[0], scale)
    assert xv.shape == (rows.numel(), C) and bool(torch.isfinite(xv.float()).all())


def test_generator_looks_like_the_problem():
    """Logit spread of several tens (50-200 on the 1000-class shapes and beyond), exponent arguments below -87 (fp32 underflow of the
    exponential is exercised), dominant and flat rows, the planted structure where B and C have room, non-uniform weights."""
    for shape in H.SHAPES:
        B, C, D = shape
        if B * C > 8_000_000:
            continue
        scale, (feats, clfs, w, logits) = _case(shape)
        ties, zero = H.planted(C, 3)
        for m in range(3):
            l = logits[m].float()
            if C % H.HF_BN:
                assert bool((l[::8].argmax(1) == C - 1).all()), f"{shape}: rows 0, 8, .. must peak on class C - 1"
            if B >= 40 and C >= 1000:
                spread = float(l.max() - l.min())
                assert 50 <= spread <= 200, f"{shape}: logit spread {spread}"
                assert float((l - l.max(1, keepdim=True).values).min()) < -88
                top = H.softmax64(logits[m]).max(1).values
                assert float(top.max()) > 0.999 and float(top.min()) < 0.5, f"{shape}: no dominant / no flat row"
            if B >= 4 * (len(ties) + 2):
                assert bool((l[1] == 0).all())                                          # all-zero features
                for i, (lo, hi) in enumerate(ties):
                    r = 4 * (i + 1) + 1
                    assert float(l[r, lo]) == float(l[r, hi]) == float(l[r].max()) and int(H.first_argmax(logits[m])[r]) == lo
                eq = l[4 * (len(ties) + 1) + 1]
                if m < 2 or zero is None:
                    assert bool((eq == 9.375).all())
                else:
                    assert float(eq[zero]) == 0 and int((eq == 9.375).sum()) == C - 1
            if zero is not None:
                assert bool((logits[2][:, zero] == 0).all()) and (B < 32 or not bool((logits[0][:, zero] == 0).all()))
        if C >= 2:
            assert float((w[1:] - w[:-1]).abs().min()) > 0.25 and float((w[:, 1:] - w[:, :-1]).abs().min()) > 0.25


def test_shape_list_reaches_every_instantiation():
    """On the 256 CUs of an MI355X the list holds softmax, raw and capped-grid cases of both tile heights and both merge forms, the
    rule's both arms and its far side, and a five-launch case in several row chunks."""
    H.assert_coverage(H.SHAPES, 256)
    with pytest.raises(AssertionError):
        H.assert_coverage([s for s in H.SHAPES if s[0] <= 256 and s[1] <= 2500], 256)       # what test_fusion_head_vs_oracle's sizes reach
    assert any(256 < B <= 512 and C <= 2048 for B, C, _ in H.SHAPES) and any(not H.head_plan(B, C) for B, C, _ in H.SHAPES)
    assert any(B * C > (32 << 20) for B, C, _ in H.SHAPES)
    for B in (1, 31, 32, 33, 63, 64, 65, 255, 256):
        for C in (1, 5, 31, 33, 127, 128, 129, 1000, 1003):
            assert any(s[:2] == (B, C) for s in H.SHAPES)


def _sub(logits, rows):
    return [l[rows] for l in logits]


@pytest.mark.parametrize("shape", H.SHAPES, ids=_ids)
def test_comparator_rejects_injected_defects(shape):
    B, C, D = shape
    scale, (feats, clfs, w, logits) = _case(shape)
    rows = _rows(B)
    logits = _sub(logits, rows)
    n = rows.numel()
    Tc = (C + H.HF_BN - 1) // H.HF_BN
    full = B >= 8                              # the all-zero feature row (row 1) is there: every tile and class is visible in it

    def verdict(got, mode):
        ref = H.reference_probs(logits, w, mode)
        tiny = H.tiny_for(w, mode)
        return H.probs_mismatch(got, ref, tiny), H.rowsum_mismatch(got, ref)

    for mode in H.MODES:
        # the faultless model passes, with room: its error is fp64 rounding
        ok = H.simulate(logits, w, mode)
        assert verdict(ok, mode) == (None, None)
        assert H.max_rel_error(ok, H.reference_probs(logits, w, mode), H.tiny_for(w, mode)) < 1e-12
        # 1. every denominator 0.1 % too large: today's cosine / 7 % criteria accept 3 %
        pm, rm = verdict(H.simulate(logits, w, mode, "denominator"), mode)
        assert pm is not None and rm is not None, f"{mode}: a row scale of 1.001 went unnoticed"
        # 2. one class tile's sum left out of the merge -- EVERY tile in turn, every classifier, single-classifier modes too
        if Tc >= 2:
            for m_bad in range(3 if mode == "fusion" else 1):
                l16 = logits[m_bad if mode == "fusion" else H.MODE_CLF[mode]]
                share = H.tile_share(l16).max(0).values
                if full:
                    assert float(share.min()) >= 2 * H.RTOL, f"{mode}: a class tile holds no visible mass in any row"
                for t in (range(Tc) if Tc <= 20 else (0, 1, Tc // 2, Tc - 2, Tc - 1)):
                    if float(share[t]) < 2 * H.RTOL:                      # (B < 8 only: the defect changes no output by the tolerance)
                        continue
                    pm, rm = verdict(H.simulate(logits, w, mode, "drop_tile", m_bad, t), mode)
                    assert pm is not None and rm is not None, f"{mode}: tile {t} of classifier {m_bad} dropped from the merge went unnoticed"
        # 3. the clamped copies of class C - 1 not masked (rows 0, 8, .. peak there)
        if C % H.HF_BN:
            pm, rm = verdict(H.simulate(logits, w, mode, "unmasked_pad"), mode)
            assert pm is not None and rm is not None, f"{mode}: unmasked padding lanes went unnoticed"
        # 4. weights of the neighbouring class / classifier for one class per tile
        if mode == "fusion" and C >= 2:
            for defect in ("w_class", "w_clf"):
                sim, ref = H.simulate(logits, w, mode, defect), H.reference_probs(logits, w, mode)
                if not full and not bool(((sim - ref).abs() > 2 * (H.RTOL * ref + H.tiny_for(w, mode))).any()):
                    continue                    # (B < 8: e.g. one row whose three classifiers agree on p = 1 -- swapped weights sum to the same)
                pm, _ = verdict(sim, mode)
                assert pm is not None, f"{defect} went unnoticed"
    # 5. a tie of the row maximum resolved to the higher column
    labels = H.xval_labels(logits[0])
    tp, n_pred = H.expected_counts(logits[0], labels)
    assert H.counts_mismatch(tp, n_pred, logits[0], labels) is None
    x = logits[0].float()
    tied = (x == x.max(1, keepdim=True).values).sum(1) > 1
    if full and C >= 2:
        assert bool(tied.any())
    if bool(tied.any()):
        cols = torch.arange(C).expand_as(x)
        last = torch.where(x == x.max(1, keepdim=True).values, cols, torch.full_like(cols, -1)).max(1).values
        bad_np = torch.bincount(last, minlength=C).to(torch.int32)
        bad_tp = torch.bincount(last[last == labels], minlength=C).to(torch.int32)
        assert H.counts_mismatch(bad_tp, bad_np, logits[0], labels) is not None
    # 6. one logit one fp16 step off: the bit comparison always sees it; the probabilities see it wherever the step is 2^-7 or more
    for m in range(3):
        x = logits[m].float()
        r = 0
        cand = (x[r].abs() >= 8) & (x[r] < x[r].max())
        c = int(torch.where(cand, x[r], torch.full_like(x[r], -math.inf)).argmax()) if bool(cand.any()) else int(x[r].argmax())
        moved = H.step_fp16(logits[m], r, c)
        msg = H.logits_mismatch(moved, logits[m])
        assert msg is not None and f"({r}, {c})" in msg
        assert H.logits_mismatch(logits[m].clone(), logits[m]) is None
        if bool(cand.any()):
            md = {0: "multimodal", 1: "vision", 2: "text"}[m]
            lg = list(logits)
            lg[m] = moved
            ref = H.reference_probs(logits, w, md)
            if float(ref[r, c]) > 1e-30:
                assert H.probs_mismatch(H.reference_probs(lg, w, md), ref, H.tiny_for(w, md)) is not None, f"{md}: a logit one fp16 step off went unnoticed"


def test_comparator_accepts_the_derived_error():
    """The comparator is not vacuous the other way either: an fp32 evaluation of the same softmax (torch's own exp and sums) stays
    inside rtol -- by a factor that leaves room for the kernel's x * log2(e) step."""
    for shape in ((256, 1000, 128), (40, 2500, 512), (33, 129, 256)):
        scale, (feats, clfs, w, logits) = _case(shape)
        for mode in H.MODES:
            ref = H.reference_probs(logits, w, mode)
            ms = (0, 1, 2) if mode == "fusion" else (H.MODE_CLF[mode],)
            got = torch.zeros(ref.shape)
            for m in ms:
                x = logits[m].float()
                e = (x - x.max(1, keepdim=True).values).exp()
                p = e * (1.0 / e.sum(1, keepdim=True))
                got += p * w[:, m] if mode == "fusion" else p
            tiny = H.tiny_for(w, mode)
            assert H.probs_mismatch(got, ref, tiny) is None and H.rowsum_mismatch(got, ref) is None
            assert H.max_rel_error(got, ref, tiny) < 2e-5
