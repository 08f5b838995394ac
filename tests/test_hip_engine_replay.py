"""The engine against a kernel-by-kernel replay of its own launch sequences (engine_replay.py): the second of the three links.  For every
case of the table an Engine is finalized with the case's reserve, the case's options are set, the entry point is called, and the same
launches are made one by one through the debug hooks on the same inputs and weights (the derived layouts rebuilt in torch).  The two
outputs are compared as int16 / int32 bit patterns: no tolerance.  A mismatch names the count, the first (row, column), got against
want and the case's plan; each geometry also runs with one block and with two, so the first of the two to fail names the block.

Sensitivity: for every mutation whose step the case runs (engine_replay.MUTATIONS), the mutated replay must differ from the engine's
output in at least one bit -- otherwise the case's inputs do not exercise that wire.

Each test prints its seconds.  Needs an MI355X: run with `pytest -m gpu`.
"""
import ctypes
import time

import pytest
import torch

import engine_replay as ER
import gemm_exact as G

pytestmark = pytest.mark.gpu

_KERNEL = {"t128": 1, "s64": 2, "v5": 3}      # GemmKernel (csrc/gemm_route.h)


@pytest.fixture(scope="module")
def gpu():
    from ovmr_amd import runtime
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    state = {"lib": runtime.load_library(), "engines": {}, "weights": {}, "n_cu": torch.cuda.get_device_properties(0).multi_processor_count}
    yield state
    state["engines"].clear()
    state["weights"].clear()
    torch.cuda.empty_cache()


def _engine(gpu, case):
    """One Engine per spec, finalized anew for the case's reserve, every option of the table set (the case's, else the default)."""
    from ovmr_amd.runtime import Engine
    if case.spec not in gpu["engines"]:
        sd, pl = ER.state_dicts(case.spec)
        e = Engine(ER.SPECS[case.spec], ER.N_CTX)
        e.load_state_dict(sd, pl)
        gpu["engines"][case.spec] = e
        gpu["weights"][case.spec] = {k: v.cuda() for k, v in ER.weights(case.spec, lambda t: t.half(), lambda t: t.float()).items()}
    e = gpu["engines"][case.spec]
    e.finalize(*case.reserve)
    for k, v in ER.options(case).items():
        e.set_option(k, v)
    return e


def _call(e, case, inp):
    """The case's entry point -> the outputs, flat."""
    a = case.args
    if case.path == "image":
        return [e.encode_image(inp["image"].cuda(), normalize=bool(a.get("normalize", 1)))]
    if case.path == "gen":
        feats = inp["feats"].cuda()
        if a["uniform"]:
            return [e.generate_tokens(feats.view(len(a["shots"]), a["shots"][0], -1))]
        return [e.generate_tokens_ragged(feats, list(a["shots"]))]
    if case.entry == "encode_text_ensemble":
        return [e.encode_text_ensemble(inp["ids"], seq_lens=list(a["seq_lens"]))]
    groups = a["groups"]
    if case.entry == "encode_text_ids":
        return [e.encode_text_ids(inp["ids0"], seq_len=groups[0][2], normalize=groups[0][3])]
    if case.entry == "encode_text_embedded":
        return [e.encode_text_embedded(inp["prompts0"], inp["index0"], seq_len=groups[0][2], normalize=groups[0][3])]
    return e.encode_text_groups([{"ids": inp[f"ids{i}"], "seq_len": Ls, "normalize": nm} if kind == "ids" else
                                 {"prompts": inp[f"prompts{i}"], "index": inp[f"index{i}"], "seq_len": Ls, "normalize": nm}
                                 for i, (kind, N, Ls, nm) in enumerate(groups)])


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _replay(gpu, case, inp, shapes, mut=None):
    be = ER.Hooks(gpu["lib"], gpu["weights"][case.spec], inp, gpu["n_cu"])
    outs = ER.run(be, case, mut)
    torch.cuda.synchronize()
    return [be.buf[o][:s.numel()].view(s.shape) for o, s in zip(outs, shapes)], be


def _mismatch(got, want):
    """None where the bit patterns agree, else the count, the first (row, column) and the two values there."""
    bad = _bits(got) != _bits(want)
    n = int(bad.sum())
    if n == 0:
        return None
    cols = got.shape[-1]
    i = int(bad.reshape(-1).nonzero()[0])
    g, w = got.reshape(-1)[i:i + 1], want.reshape(-1)[i:i + 1]
    return (f"{n} of {bad.numel()} elements differ, the first at (row {i // cols}, column {i % cols}): the engine has {float(g)!r} "
            f"({int(_bits(g)):#x}), the replay {float(w)!r} ({int(_bits(w)):#x})")


def _check_routes(gpu, case, plan):
    """The planner's restatements against the library's exports: the kernel family of every fp16 GEMM (which the fold decision is read
    from) and the kernel of every fp16 attention launch."""
    out = (ctypes.c_int * 10)()
    for r in plan:
        if r["hook"] == "gemm" and not r["f32"]:
            gpu["lib"].ovmr_debug_gemm_route(r["variant"], r["M"], r["N"], r["K"], r["epi"], r["ldc"], r["ldc"], int(r.get("stats") is not None), 0, out)
            assert out[0] == _KERNEL[r["route"][0]], (r, list(out))
        if r["hook"] in ("attention", "attention_q") and not r.get("f32"):
            assert gpu["lib"].ovmr_debug_attention_route(r["variant"], r["L"], r.get("Lq", r["L"]), r["causal"]) == r["route"], r
    rows = {(r["M"], r["D"]) for r in plan if r["hook"] == "lnfold"}
    for M, W in rows | {(r["M"], r["K"]) for r in plan if r["hook"] == "gemm" and not r["f32"] and r["epi"] == G.EPI_BIAS and r["N"] == 3 * r["K"]}:
        gpu["lib"].ovmr_debug_gemm_route(8, M, W, W, G.EPI_BIAS_RES, W, W, 0, 0, out)
        assert (out[0] == _KERNEL["s64"]) == (G.route(8, M, W, W, G.EPI_BIAS_RES)[0] == "s64"), (M, W)


@pytest.mark.parametrize("name", [c.name for c in ER.CASES])
def test_engine_equals_replay(gpu, name):
    case, t0 = ER.BY_NAME[name], time.time()
    inp = ER.inputs(case)
    e = _engine(gpu, case)
    if case.path == "image":
        assert e.encode_plan(case.args["B"]) == ER.encode_plan(case, gpu["n_cu"]), name
    got = [g.clone() for g in _call(e, case, inp)]
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(g.float()).all()) for g in got), name
    dev = {k: v.cuda() for k, v in inp.items()}
    want, be = _replay(gpu, case, dev, got)
    assert not be.hit
    _check_routes(gpu, case, be.plan)
    for i, (g, w) in enumerate(zip(got, want)):
        msg = _mismatch(g, w)
        assert msg is None, f"{name}, output {i}: {msg}\nthe plan:\n{ER.show_plan(be.plan)}"
    t1 = time.time()
    # sensitivity: every planted slip whose step runs shows in the bits
    muts = ER.mutations_of(case, gpu["n_cu"])
    assert muts, name
    for m in muts:
        mutated, bm = _replay(gpu, case, dev, got, m)
        assert bm.hit
        assert any(_mismatch(g, w) is not None for g, w in zip(got, mutated)), \
            f"{name}: the replay with '{ER.MUTATIONS[m]}' still equals the engine: the case does not exercise that wire"
    print(f"\n{name}: bit-equal over {sum(g.numel() for g in got)} elements in {t1 - t0:.2f} s; {len(muts)} mutations detected in {time.time() - t1:.2f} s")
