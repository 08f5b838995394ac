"""ovmr_fused_logits_all (EVAL_MODE all): the four eval modes of trainers/mm_classifier_one_prompt.py:348-363 from one pass over the head,
held to its contract -- plane p is BIT-EQUAL to ovmr_fused_logits(mode = p) on the same handle, options and operands.

Operands and comparators are head_exact.py's (every fp16 logit is one known number), the implementations are the list of
test_hip_head_exact.py: the one-launch head at its full grid and capped at 1, 3 and Tc + 1 workgroups (recompute queue), the entry rule,
five launches under GEMM variants 0, 6, 8, 9.  Per shape and implementation:

  * every plane against the existing single-mode entry point, as int32 bits (never against another all-modes call);
  * every plane against the fp64 softmax of the expected logits, |got - ref| <= 1e-4 * ref + tiny, and the row sums (head_exact.RTOL:
    the new launch is held to the fp64 statement directly);
  * the output is ONE sentinel-filled buffer, planes (B + 64) * C floats apart: the 64 rows behind every plane keep the sentinel;
  * the same call twice is bit-equal, and a fusion call in between equals itself before and after (the device counters re-arm across the
    two entry points).

test_shapes_reach_every_instantiation FAILS if, on the device at hand, the list lacks a tile height, a merge form, a capped grid of
either, an arm of the entry rule or a store arm.  Needs an MI355X: run with `pytest -m gpu`.
"""
import pytest
import torch

import head_exact as H
import test_hip_head_exact as T

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 128), (33, 129, 128), (65, 1003, 512), (256, 1000, 512), (40, 2048, 128), (40, 2049, 256), (256, 2500, 128),
          (520, 2048, 256), (256, 10000, 256), (300, 4500, 256), (513, 1000, 512),
          (520, 2049, 256)]             # 64-row tiles with a class count that is no multiple of 4: the scalar store arm of that kernel
CHUNKED = (1540, 21841, 128)            # B * C > 32 Mi logits: the five-launch path runs it in two row chunks
PAD_ROWS = T.PAD_ROWS


def _sentinel_planes(B, C):
    """One sentinel-filled buffer of four planes (B + PAD_ROWS) * C floats apart; the [4, B, C] view the call writes."""
    flat = torch.empty(4 * (B + PAD_ROWS) * C, dtype=torch.float32, device="cuda")
    flat.view(torch.int32).fill_(T.SENTINEL32)
    return flat, flat.view(4, B + PAD_ROWS, C)[:, :B]


def _pads_untouched(flat, B, C):
    pads = flat.view(torch.int32).view(4, B + PAD_ROWS, C)[:, B:]
    return bool((pads == T.SENTINEL32).all())


def _options(e, fused, cap, gv):
    e.set_option("fused_head", fused)
    e.set_option("head_max_grid", cap)
    e.set_option("gemm", gv)


def _case(B, C, D):
    e = T._engine(D)
    T._reset(e)
    feats, clfs, w, logits = H.exact_head_case(B, C, D, 3, e.logit_scale, B + C)
    return e, feats.cuda(), [c.cuda() for c in clfs], w, w.cuda(), [l.cuda() for l in logits]


def _check_planes(e, fd, cd, w, wd, refs, B, C, what):
    """One all-modes call under the options in force against the four single-mode calls and the fp64 references; returns the planes."""
    flat, out = _sentinel_planes(B, C)
    got = e.fused_logits_all(fd, cd[0], cd[1], cd[2], wd, out=out)
    assert got.data_ptr() == flat.data_ptr() and got.stride(0) == (B + PAD_ROWS) * C
    for p, mode in enumerate(H.MODES):
        single = e.fused_logits(fd, cd[0], cd[1], cd[2], wd, mode)
        torch.cuda.synchronize()
        same = torch.equal(got[p].view(torch.int32), single.view(torch.int32))
        assert same, f"{what}: plane {p} is not bit-equal to mode {mode}: {H.probs_mismatch(got[p], single.double(), 0.0, 0.0)}"
        tiny = H.tiny_for(w, mode)
        print(f"{what}, plane {p} ({mode}): largest relative error {H.max_rel_error(got[p], refs[mode], tiny):.2e}")
        msg = H.probs_mismatch(got[p], refs[mode], tiny)
        assert msg is None, f"{what}, plane {p} ({mode}): {msg}"
        msg = H.rowsum_mismatch(got[p], refs[mode])
        assert msg is None, f"{what}, plane {p} ({mode}): {msg}"
    assert _pads_untouched(flat, B, C), f"{what}: wrote behind row {B} of a plane"
    return got


def test_plane_order():
    from ovmr_amd import runtime
    assert runtime.ALL_MODES == H.MODES and [runtime.MODES[m] for m in runtime.ALL_MODES] == [0, 1, 2, 3]


def test_shapes_reach_every_instantiation():
    """32- and 64-row tiles, each with the local and the duty merge, at full and capped grids -- on THIS device; both arms of the entry
    rule; the float4 and the scalar store arm."""
    H.assert_coverage(SHAPES, T._n_cu())
    assert {bool(H.head_plan(B, C)) for B, C, _ in SHAPES} == {True, False}                  # one launch / five launches under the entry rule
    assert {C % 4 == 0 for _, C, _ in SHAPES} == {True, False}
    # every all-modes kernel: (tile rows, store arm) for the one-launch head
    arms = {(H.tile_rows(B, C, D, T._n_cu()), C % 4 == 0) for B, C, D in SHAPES}
    assert arms == {(32, True), (32, False), (64, True), (64, False)}, arms


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_all_modes_exact(shape):
    B, C, D = shape
    e, fd, cd, w, wd, ld = _case(B, C, D)
    bm, Tc = H.tile_rows(B, C, D, T._n_cu()), (C + H.HF_BN - 1) // H.HF_BN
    where = f"B={B} C={C} D={D} ({bm}-row tiles, {Tc} class tiles, {'duty' if Tc > 16 else 'local'} merge)"
    refs = {mode: H.reference_probs(ld, wd, mode) for mode in H.MODES}         # computed once, shared by the implementations
    try:
        for tag, fused, cap, gv in T._implementations(C):
            _options(e, fused, cap, gv)
            what = f"{tag} (fused_head {fused}, head_max_grid {cap}, gemm {gv}), {where}"
            a = _check_planes(e, fd, cd, w, wd, refs, B, C, what).clone()
            # ---- twice in a row, with a fusion call of the existing entry point in between
            f0 = e.fused_logits(fd, cd[0], cd[1], cd[2], wd, "fusion").clone()
            b = e.fused_logits_all(fd, cd[0], cd[1], cd[2], wd).clone()
            f1 = e.fused_logits(fd, cd[0], cd[1], cd[2], wd, "fusion").clone()
            c = e.fused_logits_all(fd, cd[0], cd[1], cd[2], wd)
            torch.cuda.synchronize()
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(b.view(torch.int32), c.view(torch.int32)), \
                f"{what}: two all-modes calls differ"
            assert torch.equal(f0.view(torch.int32), f1.view(torch.int32)) and torch.equal(f0.view(torch.int32), a[0].view(torch.int32)), \
                f"{what}: a fusion call between two all-modes calls differs from itself"
    finally:
        T._reset(e)


def test_row_chunks():
    """B * C > 32 Mi logits: ovmr_fused_logits_all's row-chunk loop (five launches, GEMM variant 8) advances every plane by b0 * C."""
    B, C, D = CHUNKED
    e, fd, cd, w, wd, ld = _case(B, C, D)
    assert not H.head_plan(B, C) and B * C > 32 * 1024 * 1024
    try:
        _options(e, 0, 0, 8)
        flat, out = _sentinel_planes(B, C)
        got = e.fused_logits_all(fd, cd[0], cd[1], cd[2], wd, out=out)
        for p, mode in enumerate(H.MODES):                                    # one plane's comparison tensors at a time (~1.3 GB in all)
            single = e.fused_logits(fd, cd[0], cd[1], cd[2], wd, mode)
            torch.cuda.synchronize()
            assert torch.equal(got[p].view(torch.int32), single.view(torch.int32)), f"plane {p} is not bit-equal to mode {mode}"
            del single
            ref, tiny = H.reference_probs(ld, wd, mode), H.tiny_for(w, mode)
            print(f"plane {p} ({mode}): largest relative error {H.max_rel_error(got[p], ref, tiny):.2e}")
            msg = H.probs_mismatch(got[p], ref, tiny) or H.rowsum_mismatch(got[p], ref)
            assert msg is None, f"plane {p} ({mode}): {msg}"
            del ref
        assert _pads_untouched(flat, B, C), f"wrote behind row {B} of a plane"
    finally:
        T._reset(e)


def test_argument_errors():
    """Bad arguments return OVMR_E_ARG and write nothing."""
    from ovmr_amd import runtime
    B, C, D = 33, 129, 128
    e, fd, cd, w, wd, ld = _case(B, C, D)
    flat, out = _sentinel_planes(B, C)
    lib, stride = e.lib, (B + PAD_ROWS) * C
    P, st = runtime._ptr, runtime._stream()

    def call(feats=fd, mm=cd[0], v=cd[1], t=cd[2], ww=wd, classes=C, o=out, ps=stride, h=e.h, rows=B):
        return lib.ovmr_fused_logits_all(h, P(feats), rows, P(mm), P(v), P(t), P(ww), classes, P(o), ps, st)

    bad = {"NULL handle": dict(h=None), "NULL features": dict(feats=None), "NULL multimodal classifier": dict(mm=None),
           "NULL vision classifier": dict(v=None), "NULL text classifier": dict(t=None), "NULL w": dict(ww=None), "NULL output": dict(o=None),
           "plane_stride < B * C": dict(ps=B * C - 1), "plane_stride 0": dict(ps=0), "C < 1": dict(classes=0), "B < 0": dict(rows=-1)}
    for name, kw in bad.items():
        rc = call(**kw)
        torch.cuda.synchronize()
        assert rc != 0, f"{name}: accepted"
        assert bool((flat.view(torch.int32) == T.SENTINEL32).all()), f"{name}: the output was written"
    assert call(rows=0) == 0                                                  # B == 0: nothing to do
    torch.cuda.synchronize()
    assert bool((flat.view(torch.int32) == T.SENTINEL32).all())
    with pytest.raises(runtime.OvmrError):
        e._ck(call(ww=None), "ovmr_fused_logits_all")
    assert call() == 0                                                        # and the good call still runs
    torch.cuda.synchronize()
    assert not bool((out.view(torch.int32) == T.SENTINEL32).any()) and _pads_untouched(flat, B, C)
