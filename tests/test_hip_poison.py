"""Every pass held to its inputs: the result of a call is a function of that call's inputs and weights, and of nothing else that happens
to lie in memory (poison.py: the four fills, the guarded allocator; test_poison_cpu.py: what each fill catches).  Everything is compared
as bit patterns; the one tolerance here, 6e-3 against the fp64 statement in (d), is test_attention_f16's.

  a. every case of engine_replay.CASES -- image, text ids / embedded / groups / ensemble, the uniform and the ragged generator, the
     130-row class, the one-block specs in which nothing a previous block wrote can hide the poison -- runs through its entry point
     over a workspace filled (ovmr_debug_fill_workspace) with each of the four patterns: finite, and bit-equal to each other;
  b. the last vision block with Q projected for the CLS rows only (last_q_cls = 1, at least 256 images; the replay table pins 0 there):
     tiny1 and tiny at 257 images, small1 at 256, ln_fold 0 and 1 -- the same equality, and bit-equal to last_q_cls = 0;
  c. the debug hooks over guarded operands: engine_replay.Hooks(fill=f) puts every scratch buffer, weight, input and offset table into a
     poison.Arena -- one 256-row tile of the widest row of the fill in front and behind, the scratch itself starting as the fill.  For the
     smallest case (fewest launches) of every (path, geometry family), and then for the smallest case that launches a kernel (hook,
     epilogue, route) none of those has launched, the four replays are bit-equal to each other and to the engine's output from (a), and
     no guard has been written to.  That is every kernel the towers and the generator launch behind read guards, without a
     per-kernel table;
  d. ovmr_debug_attention_q with the Q slots of the rows >= Lq overwritten by each fill (the lead: the kernels clamped a tile's spare
     query rows to L - 1, not Lq - 1, and in variants 1 and 5 a spare row votes on moving the softmax reference): the Lq output rows
     are bit-equal across the fills, bit-equal to the launch whose slots hold the true Q, and within 6e-3 of _ref_attention;
  e. the head on four shapes of head_exact.SHAPES (32- and 64-row tiles, local and duty merge): features, classifiers, w, labels and
     outputs in arenas, the workspace filled before every call; every implementation of test_hip_head_exact -- probabilities in all four
     modes, zero-shot logits, cross-validation counts -- passes head_exact's comparators and is bit-equal across the fills.

Each test prints its seconds.  On an MI355X (256 CUs), each module in a pytest run of its own, same session, three runs each: this
module 8.5 - 9.2 s (165 tests), test_hip_engine_replay.py 7.8 - 8.3 s (105 tests).  Both spend 4.7 s building the same nine engines
(the synthetic state dicts); of the rest, (a) takes 0.3 s, (b) 0.06 s, (c) 0.44 s for its 25 cases, (d) 0.05 s, (e) 0.6 s (most of it
head_exact's operands and fp64 references) against the replay's 0.75 s.  The module is NOT within the replay's figure: it is over by
about 0.7 s, and (a) + (e) alone already are by 0.2 s, so thinning (c) to one case per path (0.06 s) would not bring it under;
(c) therefore keeps the cases that put every kernel behind guards, with a spec's guarded weights shared by its cases (0.9 -> 0.44 s).
Needs an MI355X: run with `pytest -m gpu`.
"""
import ctypes
import functools
import re
import time

import pytest
import torch

import engine_replay as ER
import head_exact as H
import poison as P

pytestmark = pytest.mark.gpu

FILLS = list(P.FILLS)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def gpu():
    from ovmr_amd import runtime
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    state = {"lib": runtime.load_library(), "engines": {}, "weights": {}, "out": {},
             "n_cu": torch.cuda.get_device_properties(0).multi_processor_count}
    yield state
    state["placed"] = None
    for k in ("engines", "weights", "out"):
        state[k].clear()
    torch.cuda.empty_cache()


def _poison_workspace(lib, e, fill):
    rc = lib.ovmr_debug_fill_workspace(e.h, P.FILLS[fill], _stream())
    assert rc == 0, f"ovmr_debug_fill_workspace({fill}) returned {rc}"


def _all_equal(outs, what):
    """outs: fill -> list of tensors.  Finite under every fill and bit-equal to the outputs under `zero`."""
    for f in FILLS:
        for i, (g, z) in enumerate(zip(outs[f], outs["zero"])):
            assert bool(torch.isfinite(g.float()).all()), f"{what}, output {i}: not finite under the fill '{f}'"
            msg = P.same_bits(g, z, (f"the pass over '{f}'", "the pass over 'zero'"))
            assert msg is None, f"{what}, output {i}: {msg}"


# ---- a. the engine over a poisoned arena ----------------------------------------------------------------------------------------------

def _engine_outputs(gpu, case):
    """The case's outputs, the same under all four fills of the workspace (asserted); computed once per session."""
    import test_hip_engine_replay as TR
    if case.name not in gpu["out"]:
        inp = ER.inputs(case)
        e = TR._engine(gpu, case)                             # finalized for the case's reserve, every option of the table set
        outs = {}
        for f in FILLS:
            _poison_workspace(gpu["lib"], e, f)
            outs[f] = [g.clone() for g in TR._call(e, case, inp)]
            torch.cuda.synchronize()
        _all_equal(outs, case.name)
        gpu["out"][case.name] = outs["zero"]
    return gpu["out"][case.name]


@pytest.mark.parametrize("name", [c.name for c in ER.CASES])
def test_engine_over_poisoned_workspace(gpu, name):
    t0 = time.time()
    out = _engine_outputs(gpu, ER.BY_NAME[name])
    print(f"\n{name}: {sum(o.numel() for o in out)} elements bit-equal under {', '.join(FILLS)} in {time.time() - t0:.2f} s")


# ---- b. the CLS-only last block ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec,n_img", [("tiny1", 257), ("tiny", 257), ("small1", 256)])
@pytest.mark.parametrize("fold", [0, 1])
def test_cls_only_last_block_over_poisoned_workspace(gpu, spec, n_img, fold):
    import test_hip_engine_replay as TR
    t0 = time.time()
    outs = {}
    g = torch.Generator().manual_seed(n_img + fold)
    R = ER.SPECS[spec].image_resolution
    img = torch.randn((n_img, 3, R, R), generator=g).half().cuda()
    for q in (1, 0):
        case = ER._img(f"img_{spec}_b{n_img}_q{q}_fold{fold}", spec, n_img, opts={"last_q_cls": q, "ln_fold": fold})
        e = TR._engine(gpu, case)
        assert e.encode_plan(n_img) == [n_img]                # ONE launch sequence of at least 256 images: the CLS-only regime
        outs[q] = {}
        for f in FILLS:
            _poison_workspace(gpu["lib"], e, f)
            outs[q][f] = [e.encode_image(img, normalize=False).clone()]
            torch.cuda.synchronize()
        _all_equal(outs[q], f"{case.name}")
    msg = P.same_bits(outs[1]["zero"][0], outs[0]["zero"][0], ("last_q_cls = 1", "last_q_cls = 0"))
    assert msg is None, f"{spec}, {n_img} images, ln_fold {fold}: {msg}"
    print(f"\n{spec}, {n_img} images, ln_fold {fold}: last_q_cls 1 and 0 bit-equal under {', '.join(FILLS)} in {time.time() - t0:.2f} s")


# ---- c. the hooks over guarded operands ------------------------------------------------------------------------------------------------------

def _family(case):
    """(path, spec without its block-count suffix): tiny1 -> tiny, small2 -> small, b16x2 -> b16, head768x1 -> head768."""
    return case.path, re.sub(r"(x\d+|(?<=[a-z])\d)$", "", case.spec)


@functools.lru_cache(maxsize=None)
def _plan(name, n_cu=ER.N_CU):
    return ER.plan(ER.BY_NAME[name], n_cu)


def _kernels(case, n_cu=ER.N_CU):
    """What the case launches: (hook, fp32?, epilogue, route) of every step."""
    return {(r["hook"], r.get("f32"), r.get("epi"), r.get("qgelu"), str(r.get("route")), str(r.get("route1"))) for r in _plan(case.name, n_cu)}


@functools.lru_cache(maxsize=None)
def hook_cases(n_cu=ER.N_CU):
    """The smallest case (fewest launches; the table's order breaks ties) of every (path, geometry family), then, smallest first, every
    case that launches a kernel none of the chosen has launched."""
    cost = {c.name: len(_plan(c.name, n_cu)) for c in ER.CASES}
    order = sorted(ER.CASES, key=lambda c: cost[c.name])      # (stable: the table's order among equals)
    chosen, seen = [], set()
    for fam in dict.fromkeys(_family(c) for c in ER.CASES):
        c = next(c for c in order if _family(c) == fam)
        chosen.append(c.name)
        seen |= _kernels(c, n_cu)
    for c in order:
        k = _kernels(c, n_cu)
        if c.name not in chosen and not k <= seen:
            chosen.append(c.name)
            seen |= k
    return sorted(chosen, key=lambda n: list(ER.SPECS).index(ER.BY_NAME[n].spec))      # spec by spec: one spec's guarded weights at a time


@pytest.mark.parametrize("name", hook_cases())
def test_hooks_over_guarded_operands(gpu, name):
    import test_hip_engine_replay as TR
    case, t0 = ER.BY_NAME[name], time.time()
    want = _engine_outputs(gpu, case)
    TR._engine(gpu, case)                                     # (the spec's weights on the device)
    if gpu.get("placed_spec") != case.spec:                   # the weights of ONE spec, guarded once per fill (the cases come spec by spec)
        gpu["placed"], gpu["placed_spec"] = None, case.spec
        w = gpu["weights"][case.spec]
        gpu["placed"] = {f: P.Arena(f, "cuda", P.guard_elems(ER.Hooks.widest_row(w))).place_all(w) for f in FILLS}
    dev = {k: v.cuda() for k, v in ER.inputs(case).items()}
    for f in FILLS:
        be = ER.Hooks(gpu["lib"], gpu["placed"][f], dev, gpu["n_cu"], fill=f)
        outs = ER.run(be, case)
        torch.cuda.synchronize()
        assert not be.hit
        for i, (o, w) in enumerate(zip(outs, want)):
            got = be.buf[o][:w.numel()].view(w.shape)
            assert bool(torch.isfinite(got.float()).all()), f"{name}, output {i}: the replay over '{f}' is not finite"
            msg = P.same_bits(got, w, (f"the replay over guarded operands under '{f}'", "the engine"))
            assert msg is None, f"{name}, output {i}: {msg}\nthe plan:\n{ER.show_plan(be.plan)}"
        assert be.arena.intact(), f"{name}: a launch of the replay under '{f}' wrote into a guard\nthe plan:\n{ER.show_plan(be.plan)}"
        del be
    assert gpu["placed"]["big"].arena.intact(), f"{name}: a launch of the replay wrote into the guard of a weight"
    print(f"\n{name}: {len(_plan(name, gpu['n_cu']))} launches over guarded operands, bit-equal to the engine under {', '.join(FILLS)} "
          f"in {time.time() - t0:.2f} s")


# ---- d. attention_q with stale query rows -------------------------------------------------------------------------------------------------

ATT_B, ATT_H = 3, 3                     # 9 (sequence, head) pairs: the last XCD slot of variants 1 / 5 runs through its early return
ATT_LQ = (1, 17)


@functools.lru_cache(maxsize=None)
def _attention_case(L):
    """qkv as test_attention_f16 builds it (fp16 normals, one key spiked x 6 at L // 2 and, for L >= 256, one x 9 at L - 70: the lazy
    reference moves), the spikes in the first and in the last sequence; and the fp64 statement for the first max(ATT_LQ) queries."""
    from test_hip_kernels import _ref_attention
    B, Hh, D = ATT_B, ATT_H, ATT_H * 64
    g = torch.Generator().manual_seed(B * L + Hh)
    qkv = torch.randn(B * L, 3 * D, generator=g).half()
    for b in (0, B - 1):
        qkv[b * L + L // 2, D:D + 64] *= 6.0
        if L >= 256:
            qkv[b * L + L - 70, D:D + 64] *= 9.0
    ref = _ref_attention(qkv.float(), B, L, Hh, 0).view(B, L, D)[:, :max(ATT_LQ)].contiguous()
    return qkv, ref


@pytest.mark.parametrize("variant", [0, 1, 3, 5])
@pytest.mark.parametrize("Lq", ATT_LQ)
@pytest.mark.parametrize("L", [197, 257, 577])
def test_attention_q_ignores_stale_query_rows(gpu, L, Lq, variant):
    t0 = time.time()
    B, Hh, D = ATT_B, ATT_H, ATT_H * 64
    qkv, ref = _attention_case(L)
    ref = ref[:, :Lq].reshape(B * Lq, D)

    def launch(fill, stale):
        arena = P.Arena(fill, "cuda", P.guard_elems(3 * D))
        x = arena.place(qkv)
        if stale:                                             # the Q slots of the rows >= Lq of every sequence: the 16-bit half of the pattern
            x.view(B, L, 3 * D)[:, Lq:, :D] = P.fill_(torch.empty(1, dtype=torch.float16, device="cuda"), fill)
        out = arena.take(B * Lq * D, "f16")
        rc = gpu["lib"].ovmr_debug_attention_q(variant, _p(x), _p(out), B, L, Lq, Hh, 0, _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert arena.intact(), f"variant {variant}, L = {L}, Lq = {Lq}, fill '{fill}': the launch wrote into a guard"
        return out.clone().view(B * Lq, D)

    kernel = gpu["lib"].ovmr_debug_attention_route(variant, L, Lq, 0)
    what = f"variant {variant} (kernel {kernel}), L = {L}, Lq = {Lq}"
    true_q = launch("zero", stale=False)
    err = float((true_q.float().cpu() - ref).abs().max())
    print(f"\n{what}: max |error| against fp64 {err:.2e}")
    assert bool(torch.isfinite(true_q.float()).all()) and err < 6e-3, f"{what}: max err {err}"
    for f in FILLS:
        got = launch(f, stale=True)
        msg = P.same_bits(got, true_q, (f"stale Q slots of '{f}'", "the true Q in the slots"))
        assert msg is None, f"{what}: {msg}"
    print(f"{what}: bit-equal under {', '.join(FILLS)} and to the true Q in {time.time() - t0:.2f} s")


# ---- e. the head --------------------------------------------------------------------------------------------------------------------------

HEAD_SHAPES = [(40, 2048, 128), (40, 2049, 256), (520, 2048, 256), (300, 4500, 256)]


def _missing(shapes, n_cu):
    """How many instantiations H.assert_coverage asks for the shapes do not reach on n_cu compute units."""
    soft, capped, raw = H.coverage(shapes, n_cu)
    want = {(32, "local"), (32, "duty"), (64, "local"), (64, "duty")}
    return len(want - soft) + len(want - capped) + len({32, 64} - raw)


def head_shapes(n_cu):
    """The four shapes; on a device where they do not reach every instantiation, the next shapes of H.SHAPES that repair it."""
    shapes = list(HEAD_SHAPES)
    for s in H.SHAPES:
        if not _missing(shapes, n_cu):
            break
        if s not in shapes and _missing(shapes + [s], n_cu) < _missing(shapes, n_cu):
            shapes.append(s)
    return shapes


def test_head_shapes_reach_every_instantiation():
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    H.assert_coverage(head_shapes(n_cu), n_cu)
    assert head_shapes(256) == HEAD_SHAPES


@pytest.mark.parametrize("i", range(len(HEAD_SHAPES)))
def test_head_over_poisoned_workspace_and_guarded_operands(gpu, i):
    import test_hip_head_exact as TH
    shapes = head_shapes(gpu["n_cu"])
    for shape in [shapes[i]] + (shapes[len(HEAD_SHAPES):] if i == 0 else []):
        _head_case(gpu, TH, shape)


def _head_engine(gpu, D):
    """The head reads nothing of the model but embed_dim and the logit scale: the replay table's one-block engine of that width,
    finalized as test_hip_head_exact finalizes its own (the logits workspace does not depend on the reserve)."""
    import test_hip_engine_replay as TR
    spec = {128: "tiny1", 256: "small1", 512: "b16x1", 768: "head768x1"}[D]
    assert ER.SPECS[spec].embed_dim == D
    return TR._engine(gpu, ER.Case("head", "image", spec, {}, (64, 64, 1024), "", {}))


def _head_case(gpu, TH, shape):
    t0 = time.time()
    B, C, D = shape
    e = _head_engine(gpu, D)
    TH._reset(e)
    scale = e.logit_scale
    feats, clfs, w, logits = H.exact_head_case(B, C, D, 3, scale, B + C)
    ld, wd = [l.cuda() for l in logits], w.cuda()
    where = f"B={B} C={C} D={D} ({H.tile_rows(B, C, D, gpu['n_cu'])}-row tiles, {'duty' if (C + H.HF_BN - 1) // H.HF_BN > 16 else 'local'} merge)"
    xl = [H.xval_expected(feats.cuda(), c.cuda(), scale) for c in clfs]
    labels = [H.xval_labels(x) for x in xl]
    refs = {mode: (H.reference_probs(ld, wd, mode), H.tiny_for(w, mode)) for mode in H.MODES}
    first = {}
    try:
        for f in FILLS:
            arena = P.Arena(f, "cuda", P.guard_elems(max(C, D)))
            fd, cd, wa = arena.place(feats), [arena.place(c) for c in clfs], arena.place(w)
            la = [arena.place(l) for l in labels]
            got = {}

            def call(key, fn, elems, kind, shape_):
                _poison_workspace(gpu["lib"], e, f)
                out = arena.take(elems, kind).view(shape_)
                if kind == "i32":
                    out.zero_()                               # the counts accumulate: the caller's zeros are an input
                fn(out)
                torch.cuda.synchronize()
                got[key] = out

            for m in (0, 2):
                for tag, fused, gv in [("one launch", 1, 8)] + [(f"scale + GEMM, gemm {v}", 0, v) for v in TH.GEMMS]:
                    e.set_option("fused_head", fused)
                    e.set_option("gemm", gv)
                    call(("zeroshot", m, tag), lambda out: e.zeroshot_logits(fd, cd[m], out=out), B * C, "f16", (B, C))
            for mode in H.MODES:
                for tag, fused, cap, gv in TH._implementations(C):
                    e.set_option("fused_head", fused)
                    e.set_option("head_max_grid", cap)
                    e.set_option("gemm", gv)
                    call((mode, tag), lambda out: e.fused_logits(fd, cd[0], cd[1], cd[2], wa, mode, out=out), B * C, "f32", (B, C))
            TH._reset(e)
            for m in range(3):
                for tag, xf, gv in [("fused argmax", 1, 8)] + [(f"materialised, gemm {v}", 0, v) for v in TH.GEMMS]:
                    e.set_option("xval_fused", xf)
                    e.set_option("gemm", gv)
                    call(("xval", m, tag), lambda out: e.xval_counts(fd, la[m], cd[m], out[0], out[1]), 2 * C, "i32", (2, C))
            TH._reset(e)
            assert arena.intact(), f"{where}: a call under '{f}' wrote into a guard"
            if not first:
                # the comparators of head_exact, once: what is bit-equal to these results under the other fills passes them too
                for key, out in got.items():
                    what = f"{key}, {where}, fill '{f}'"
                    if key[0] == "zeroshot":
                        msg = H.logits_mismatch(out, ld[key[1]])
                    elif key[0] == "xval":
                        msg = H.counts_mismatch(out[0], out[1], xl[key[1]], labels[key[1]])
                    else:
                        ref, tiny = refs[key[0]]
                        msg = H.probs_mismatch(out, ref, tiny) or H.rowsum_mismatch(out, ref)
                    assert msg is None, f"{what}: {msg}"
                first = {k: v.clone() for k, v in got.items()}
            else:
                for key, out in got.items():
                    msg = P.same_bits(out, first[key], (f"the call under '{f}'", "the call under 'zero'"))
                    assert msg is None, f"{key}, {where}: {msg}"
            del arena, got
    finally:
        TH._reset(e)
    print(f"\n{where}: {len(first)} results bit-equal under {', '.join(FILLS)} in {time.time() - t0:.2f} s")
