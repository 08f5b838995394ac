"""The classifier head held to exact values: ovmr_fused_logits, ovmr_zeroshot_logits and ovmr_xval_counts on operands for which every
partial sum of every dot product is exact in fp32 (head_exact.py: the method, the planted structure, the derived tolerance).  The fp16
logits are then ONE number in any summation order, so

  * zero-shot logits are compared bit for bit with the expected fp16 logits, one-launch kernel and scale + GEMM path, every GEMM variant;
    test_zeroshot_row_chunks does so over 65536 + 33 rows, where the scale + GEMM path runs two row chunks;
  * probabilities (fusion / text / vision / multimodal) with the fp64 softmax of the expected logits weighted by w:
    |got - ref| <= 1e-4 * ref + tiny, row sums within 1e-4 -- for the one-launch head at its full grid, capped at 1, 3 and Tc + 1
    workgroups (recompute queue), as the entry rule decides, and for the five-launch path under GEMM variants 0, 6, 8, 9;
  * all one-launch grids are bit-equal to each other, the same call twice is bit-equal, one launch against five launches within 2e-4;
  * nothing behind row B of a sentinel-filled output is written (the output is dense [B, C]: a store past a row's last column lands
    in the next row or, in the last row, in the sentinel);
  * cross-validation counts (fused argmax and materialised logits, every GEMM variant) EQUAL the bincounts of the first-index argmax
    of the expected logits h(h(f . clf) * scale) -- no near-tie allowance.

test_shapes_reach_every_instantiation FAILS if, on the device at hand, the list lacks a tile height, a merge form, a capped grid of
either or a raw case of either.  Needs an MI355X: run with `pytest -m gpu`.

Largest relative probability error observed on an MI355X (256 CUs) over all cases, beside the derived 2e-5 and the bound 1e-4
(test_report_largest_errors prints the table):
    one launch (full grid and every capped grid: bit-equal)     3.75e-6   (multimodal, 1540 x 21 841, width 128)
    entry rule                                                   3.71e-6
    five launches, GEMM variants 0 / 6 / 8 / 9                   3.71e-6 each (text, 1540 x 21 841, width 128)
The two paths meet the same figure: it is the x * log2(e) product of the largest |x| <= 88 in a row whose sum is exactly 1.
"""
import pytest
import torch

import head_exact as H
from conftest import usable_threads

pytestmark = pytest.mark.gpu

MODELS = {128: "tiny", 256: "small", 512: "ViT-B/16", 768: "head768"}
GEMMS = (0, 6, 8, 9)
SENTINEL32 = 0x5A5A5A5A                 # fp32 1.5363e16: no probability, compared as bits
SENTINEL16 = 0x5A5A                     # fp16 203.25: above every logit here
PAD_ROWS = 64

_ENGINES = {}
_WORST = {}                             # implementation -> (largest relative error, case)


def _engine(D):
    """One finalized engine per embedding width (the head reads nothing of the model but embed_dim and logit_scale)."""
    if D not in _ENGINES:
        from ovmr_amd import modules, synth
        assert torch.cuda.is_available(), "GPU tests need a ROCm device"
        torch.set_num_threads(usable_threads())
        spec = synth.SPECS[MODELS[D]]
        assert spec.embed_dim == D
        sd = {k: torch.from_numpy(v) for k, v in synth.clip_state_dict(spec, 11, jitter=True).items()}
        e = modules.CLIPModel(sd, spec).engine(2)
        e.load_state_dict({}, {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, 2, 11, True).items()})
        e.finalize(64, 64, 1024)        # (the logits workspace does not depend on max_classes: 32 Mi logits per classifier)
        _ENGINES[D] = e
    return _ENGINES[D]


def _reset(e):
    for k, v in (("fused_head", 1), ("head_max_grid", 0), ("gemm", 8), ("xval_fused", 1)):
        e.set_option(k, v)


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _sentinel_out(B, C, dtype):
    flat = torch.empty((B + PAD_ROWS) * C, dtype=dtype, device="cuda")
    if dtype == torch.float32:
        flat.view(torch.int32).fill_(SENTINEL32)
    else:
        flat.view(torch.int16).fill_(SENTINEL16)
    return flat, flat[:B * C].view(B, C)


def _tail_untouched(flat, B, C):
    t = flat[B * C:]
    return bool((t.view(torch.int32) == SENTINEL32).all()) if flat.dtype == torch.float32 else bool((t.view(torch.int16) == SENTINEL16).all())


def _implementations(C):
    Tc = (C + H.HF_BN - 1) // H.HF_BN
    one = [("one launch", 2, 0, 8), ("one launch, grid 1", 2, 1, 8), ("one launch, grid 3", 2, 3, 8), ("one launch, grid Tc+1", 2, Tc + 1, 8),
           ("entry rule", 1, 0, 8)]
    return one + [(f"five launches, gemm {v}", 0, 0, v) for v in GEMMS]


def test_shapes_reach_every_instantiation():
    """launch_head_fused picks 32-row tiles while ceil(B/32) * ceil(C/128) <= CUs, else 64-row tiles; more than 16 class tiles merge in
    the duty phase.  The list must hold softmax and raw cases of both heights, capped grids of both, both merge forms -- on THIS device."""
    H.assert_coverage(H.SHAPES, _n_cu())


@pytest.mark.parametrize("shape", H.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_head_exact(shape):
    B, C, D = shape
    e = _engine(D)
    _reset(e)
    scale = e.logit_scale
    feats, clfs, w, logits = H.exact_head_case(B, C, D, 3, scale, B + C)
    bm = H.tile_rows(B, C, D, _n_cu())
    Tc = (C + H.HF_BN - 1) // H.HF_BN
    where = f"B={B} C={C} D={D} ({bm}-row tiles, {Tc} class tiles, {'duty' if Tc > 16 else 'local'} merge)"
    fd, cd, wd = feats.cuda(), [c.cuda() for c in clfs], w.cuda()
    ld = [l.cuda() for l in logits]
    assert e.head_plan(B, C) == int(H.head_plan(B, C)), where
    try:
        # ---- zero-shot logits: bit-equal, both paths, two of the classifiers (the last one holds the zero row)
        for m in (0, 2):
            for tag, fused, gv in [("one launch", 1, 8)] + [(f"scale + GEMM, gemm {v}", 0, v) for v in GEMMS]:
                e.set_option("fused_head", fused)
                e.set_option("gemm", gv)
                flat, out = _sentinel_out(B, C, torch.float16)
                z = e.zeroshot_logits(fd, cd[m], out=out)
                torch.cuda.synchronize()
                msg = H.logits_mismatch(z, ld[m])
                assert msg is None, f"zero-shot logits, {tag}, classifier {m}, {where}: {msg}"
                assert _tail_untouched(flat, B, C), f"zero-shot logits, {tag}, {where}: wrote behind row {B}"
        # ---- probabilities
        line = []
        for mode in H.MODES:
            ref = H.reference_probs(ld, wd, mode)
            tiny = H.tiny_for(w, mode)
            outs = {}
            for tag, fused, cap, gv in _implementations(C):
                e.set_option("fused_head", fused)
                e.set_option("head_max_grid", cap)
                e.set_option("gemm", gv)
                flat, out = _sentinel_out(B, C, torch.float32)
                got = e.fused_logits(fd, cd[0], cd[1], cd[2], wd, mode, out=out)
                torch.cuda.synchronize()
                what = f"{mode}, {tag} (fused_head {fused}, head_max_grid {cap}, gemm {gv}), {where}"
                err = H.max_rel_error(got, ref, tiny)
                if err >= _WORST.get(tag.split(", grid")[0], (-1.0, ""))[0]:
                    _WORST[tag.split(", grid")[0]] = (err, f"{mode} {where}")
                line.append(f"{mode[:2]}/{tag}: {err:.2e}")
                msg = H.probs_mismatch(got, ref, tiny)
                assert msg is None, f"{what}: {msg}"
                msg = H.rowsum_mismatch(got, ref)
                assert msg is None, f"{what}: {msg}"
                assert _tail_untouched(flat, B, C), f"{what}: wrote behind row {B}"
                outs[tag] = got.clone()
            base = outs["one launch"]
            for tag, fused, cap, gv in _implementations(C):
                if fused == 2 or (fused == 1 and H.head_plan(B, C)):
                    same = torch.equal(base.view(torch.int32), outs[tag].view(torch.int32))
                    assert same, f"{mode}, {where}: '{tag}' is not bit-equal to the full grid: {H.probs_mismatch(outs[tag], base.double(), 0.0, 0.0)}"
                if fused == 0:
                    d = (outs[tag].double() - base.double()).abs()
                    assert bool((d <= 2 * H.RTOL * ref + 2 * tiny).all()), f"{mode}, {where}: one launch and '{tag}' differ by more than 2 rtol"
            if not H.head_plan(B, C):               # the rule's far side runs the GEMM path: bit-equal to fused_head = 0 under the default variant
                assert torch.equal(outs["entry rule"].view(torch.int32), outs["five launches, gemm 8"].view(torch.int32)), f"{mode}, {where}"
        print(f"\n{where}: largest relative error " + "; ".join(line))
        # ---- the same call twice (the device counters re-arm themselves), full and capped grid
        for cap in (0, 3):
            e.set_option("fused_head", 2)
            e.set_option("head_max_grid", cap)
            a = e.fused_logits(fd, cd[0], cd[1], cd[2], wd, "fusion").clone()
            b = e.fused_logits(fd, cd[0], cd[1], cd[2], wd, "fusion")
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{where}: two calls in a row differ (grid cap {cap})"
        _reset(e)
        # ---- cross-validation counts: equal, fused argmax and materialised logits
        for m in range(3):
            xl = H.xval_expected(fd, cd[m], scale)
            labels = H.xval_labels(xl)
            for tag, xf, gv in [("fused argmax", 1, 8)] + [(f"materialised, gemm {v}", 0, v) for v in GEMMS]:
                e.set_option("xval_fused", xf)
                e.set_option("gemm", gv)
                counts = torch.zeros((2, C), dtype=torch.int32, device="cuda")
                e.xval_counts(fd, labels, cd[m], counts[0], counts[1])
                torch.cuda.synchronize()
                msg = H.counts_mismatch(counts[0], counts[1], xl, labels)
                assert msg is None, f"xval_counts, {tag}, classifier {m}, {where}: {msg}"
    finally:
        _reset(e)


def test_zeroshot_row_chunks():
    """ovmr_zeroshot_logits over more than 65536 rows: the scale + GEMM path runs two row chunks, the second one 33 rows (a partial
    tile) behind b0 * C logits; C = 5 is an odd ldc (rows that are not 16-byte aligned, the scalar store arm).  Bit-equal logits from
    GEMM variants 0 and 8 and from the one-launch kernel, which takes a raw call at any size."""
    B, C, D = 65536 + 33, 5, 128
    e = _engine(D)
    _reset(e)
    feats, clfs, _, logits = H.exact_head_case(B, C, D, 1, e.logit_scale, B + C)
    fd, cd, ld = feats.cuda(), clfs[0].cuda(), logits[0].cuda()
    try:
        for tag, fused, gv in (("scale + GEMM, gemm 0", 0, 0), ("scale + GEMM, gemm 8", 0, 8), ("one launch", 1, 8)):
            e.set_option("fused_head", fused)
            e.set_option("gemm", gv)
            flat, out = _sentinel_out(B, C, torch.float16)
            z = e.zeroshot_logits(fd, cd, out=out)
            torch.cuda.synchronize()
            msg = H.logits_mismatch(z, ld)
            assert msg is None, f"zero-shot logits, {tag}, B={B} C={C} D={D}: {msg}"
            assert _tail_untouched(flat, B, C), f"zero-shot logits, {tag}: wrote behind row {B}"
    finally:
        _reset(e)


def test_report_largest_errors():
    """Prints the largest relative probability error per implementation over the cases run in this session (beside the derived 2e-5)."""
    for tag, (err, case) in sorted(_WORST.items()):
        print(f"\nlargest relative error, {tag}: {err:.3e}  ({case})")
        assert err <= H.RTOL
