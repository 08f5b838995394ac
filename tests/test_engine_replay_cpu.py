"""The replay of the engine's launch sequences (engine_replay.py), on the CPU: the first of its three links -- the wiring equals the
reference model -- and the two properties the GPU test (test_hip_engine_replay.py) relies on.

  * test_wiring_equals_oracle: the `torch` backend against oracle.encode_image, encode_text / text_encoder_forward and the aggregator part
    of prompt_learner_forward, on the same jittered synthetic state dicts, for every case of the table.
  * test_cases_reach_every_branch: from plan() alone.
  * test_every_mutation_changes_the_result: each planted wiring slip moves the `torch` backend's fp64 result on every case where its
    step runs, so a replay that matches the engine rules that slip out.
"""
import time

import pytest
import torch

import engine_replay as ER
from oracle import ovmr_oracle as O

CASE_IDS = [c.name for c in ER.CASES]


def _weights(case, dt):
    return ER.weights(case.spec, lambda t: t.to(dt), lambda t: t.to(dt))


def _replay(case, dt, mut=None):
    be = ER.Torch(_weights(case, dt), ER.inputs(case), dt)
    outs = ER.run(be, case, mut)
    return [be.buf[o].clone() for o in outs], be


def _normalized(x, times):
    for _ in range(times):
        x = O.l2_normalize(x)
    return x


_ORACLE = {}


def _oracle(case, dt):
    """The oracle's outputs of the case, fed tensors of dtype dt (options and reserves do not reach it: cached without them)."""
    key = (repr(ER.input_key(case)), dt)
    if key not in _ORACLE:
        sd, pl = ER.state_dicts(case.spec)
        sd, pl = {k: v.to(dt) for k, v in sd.items()}, {k: v.to(dt) for k, v in pl.items()}
        inp, a, s = ER.inputs(case), case.args, ER.SPECS[case.spec]
        with torch.no_grad():
            if case.path == "image":
                out = [_normalized(O.encode_image(inp["image"].to(dt), sd), 1 if a.get("normalize", 1) else 0)]
            elif case.entry == "encode_text_ensemble":
                u = torch.stack([O.l2_normalize(O.encode_text(inp["ids"][t], sd)) for t in range(a["T"])])
                out = [O.l2_normalize(u.mean(dim=0))]
            elif case.path == "text":
                out = []
                for i, (kind, N, Ls, normalize) in enumerate(a["groups"]):
                    f = O.encode_text(inp[f"ids{i}"], sd) if kind == "ids" else \
                        O.text_encoder_forward(inp[f"prompts{i}"].to(dt), inp[f"index{i}"], sd, dtype=dt)
                    out.append(_normalized(f, normalize))
            else:
                D, shots, toks, r0 = s.embed_dim, a["shots"], [], 0
                for n in ([sum(shots)] if a["uniform"] else shots):          # ragged: class by class
                    Cb = len(shots) if a["uniform"] else 1
                    feats = inp["feats"][r0:r0 + n].to(dt).view(Cb, n // Cb, D)
                    zeros = torch.zeros((Cb, s.context_length, D), dtype=dt)
                    toks.append(O.prompt_learner_forward(feats, torch.zeros(Cb, dtype=torch.int64), torch.ones(Cb, dtype=torch.int32), zeros,
                                                         zeros[:1], pl, ER.N_CTX)[4])
                    r0 += n
                out = [torch.cat(toks)]
        _ORACLE[key] = [o.reshape(-1).double() for o in out]
    return _ORACLE[key]


def _distance(got, want):
    """The largest difference over the outputs, relative to the largest feature element."""
    return max(float((g.double() - w).abs().max() / w.abs().max()) for g, w in zip(got, want))


@pytest.mark.parametrize("name", CASE_IDS)
def test_wiring_equals_oracle(name):
    """Every oracle function pins a dtype -- layer_norm and multi_head_attention upcast with .float() (clip/model.py:153-159), so an oracle
    fed float64 keeps fp32 roundings and the 1e-9 of two fp64 evaluations is out of reach: measured, the fp64 replay stands 0.9e-7 to
    3.7e-7 from the oracle fed float64 (printed per case).  Both therefore run in fp32, and the bound is 8 times the distance between the
    oracle fed fp32 and fed fp64 on the case: the oracle's own fp32 error, with room for another summation order.  Measured over the 105
    cases: that distance is 2.4e-7 to 1.3e-6 of the largest feature element, the replay stands 0 to 1.0e-6 from the oracle, between 0
    and 1.29 times the distance (image 0.80 - 1.17, text 0.33 - 1.16, generator 0 - 1.29); the bound allows 8."""
    case, t0 = ER.BY_NAME[name], time.time()
    got, be = _replay(case, torch.float32)
    assert not be.hit
    o32, o64 = _oracle(case, torch.float32), _oracle(case, torch.float64)
    assert [g.numel() for g in got] == [o.numel() for o in o32]
    own = _distance(o32, o64)
    d = _distance(got, o32)
    d64 = _distance(_replay(case, torch.float64)[0], o64)
    print(f"\n{name}: replay - oracle (fp32) {d:.3e}; the oracle's fp32 - fp64 {own:.3e}; ratio {d / own:.2f} (bound 8); "
          f"fp64 replay - oracle fed fp64 {d64:.3e}; {time.time() - t0:.2f} s")
    assert own > 0 and d <= 8 * own, f"{name}: {d:.3e} from the oracle, its own fp32 error is {own:.3e}\n{ER.show_plan(be.plan)}"


# ---- every branch of the wiring, from plan() alone ----------------------------------------------------------------------------------

def _sequences(p):
    """An image plan as launch sequences: (images, patch route, folded, images of the last block's CLS launch)."""
    out = []
    for r in p:
        if r["hook"] in ("gemm_patches", "im2col"):
            out.append({"B": r["B"], "front": "fused" if r["hook"] == "gemm_patches" else "im2col_f32" if r["f32"] else "im2col_f16", "fold": False})
        elif r["hook"] == "lnfold":
            out[-1]["fold"] = True
    return out


def _passes(p):
    """A text plan as passes of groups: per pass [(kind, N, Ls)], the engine's attention launch, folded or not."""
    out, cur = [], None
    for r in p:
        if cur is None:
            cur = {"groups": [], "engine": None, "fold": False}
        if r["hook"] == "text_embed_ids":
            cur["groups"].append(("ids", r["N"], r["Lseq"]))
        elif r["hook"] == "text_add_pos":
            cur["groups"].append(("emb", r["N"], r["Lseq"]))
        elif r["hook"] == "attention":
            cur["engine"] = r.get("engine")
        elif r["hook"] == "lnfold":
            cur["fold"] = True
        elif r["hook"] == "layernorm" and r["g"] == "ln_final.weight":
            out.append(cur)
            cur = None
    return out


def _short_mixed(ps):
    g = ps["groups"]
    return 2 <= len(g) <= 4 and all(L <= 32 for _, _, L in g) and {k for k, _, _ in g} == {"ids", "emb"} and \
        len({L for _, _, L in g}) == len(g) and ps["engine"] == "one launch for the groups"


BRANCHES = {
    # image tower
    "patches gathered by the GEMM": lambda c, p: any(s["front"] == "fused" for s in _sequences(p)),
    "im2col pass, fp16 images": lambda c, p: any(s["front"] == "im2col_f16" for s in _sequences(p)),
    "im2col pass, fp32 images": lambda c, p: any(s["front"] == "im2col_f32" for s in _sequences(p)),
    "one launch sequence": lambda c, p: len(_sequences(p)) == 1,
    "several launch sequences": lambda c, p: len(_sequences(p)) > 1,
    "several launch sequences, the remainder folded into the last": lambda c, p: len(_sequences(p)) > 1 and _sequences(p)[-1]["B"] > _sequences(p)[0]["B"],
    "image tower folded": lambda c, p: any(s["fold"] for s in _sequences(p)),
    "image tower unfolded at width % 256 == 0": lambda c, p: c.path == "image" and ER.SPECS[c.spec].vision_width % 256 == 0 and not any(s["fold"] for s in _sequences(p)),
    "image tower folded, one block (row statistics alone)": lambda c, p: any(s["fold"] for s in _sequences(p)) and ER.SPECS[c.spec].vision_layers == 1,
    "last block, fewer than 256 images": lambda c, p: any(r["hook"] == "attention_q" and r["B"] < 256 for r in p),
    "last block, at least 256 images": lambda c, p: any(r["hook"] == "attention_q" and r["B"] >= 256 for r in p),
    "L = 197 under the single-pass attention kernel": lambda c, p: any(r["hook"] == "attention" and r.get("route") == 3 and r["L"] == 197 for r in p),
    "L = 197 under attention 1": lambda c, p: any(r["hook"] == "attention" and r["variant"] == 1 and r["L"] == 197 for r in p),
    # text tower
    "text tower folded": lambda c, p: any(ps["fold"] for ps in _passes(p)),
    "text tower unfolded": lambda c, p: any(not ps["fold"] for ps in _passes(p)),
    "text tower folded, several groups": lambda c, p: any(ps["fold"] and len(ps["groups"]) > 1 for ps in _passes(p)),
    "a pass of one group": lambda c, p: any(len(ps["groups"]) == 1 for ps in _passes(p)),
    "two to four short groups, ids and embedded, lengths different: one attention launch": lambda c, p: any(_short_mixed(ps) for ps in _passes(p)),
    "five groups": lambda c, p: any(len(ps["groups"]) == 5 for ps in _passes(p)),
    "a group longer than 32 among short ones": lambda c, p: any(1 < len(ps["groups"]) <= 4 and max(L for _, _, L in ps["groups"]) > 32 and
                                                                 min(L for _, _, L in ps["groups"]) <= 32 and ps["engine"] == "a launch per group" for ps in _passes(p)),
    "ids beyond max_prompts": lambda c, p: c.entry == "encode_text_ids" and len(_passes(p)) > 1,
    "embedded prompts beyond max_prompts": lambda c, p: c.entry == "encode_text_embedded" and len(_passes(p)) > 1,
    "ensemble": lambda c, p: any(r["hook"] == "text_ensemble" for r in p),
    "ensemble of more than four templates": lambda c, p: any(r["hook"] == "text_ensemble" and r["T"] > 4 for r in p),
    # generator
    "generator, uniform": lambda c, p: any(r["hook"] == "attention" and r["f32"] == 1 for r in p),
    "generator, ragged": lambda c, p: any(r["hook"] == "attention_f32_varlen" for r in p),
    "generator, one class alone": lambda c, p: c.path == "gen" and len(c.args["shots"]) == 1,
    "generator, several chunks of a ragged call": lambda c, p: sum(r["hook"] == "agg_input" for r in p) > 1 and not c.args["uniform"],
    "generator, several chunks of a uniform call": lambda c, p: sum(r["hook"] == "agg_input" for r in p) > 1 and c.args["uniform"],
    "generator, a class of more than 128 rows": lambda c, p: any(r["hook"] == "attention_f32_long" and r["max_len"] > 128 for r in p),
}
for _g in (0, 6, 8):
    for _path in ("image", "text"):
        BRANCHES[f"{_path}, gemm {_g}"] = lambda c, p, g=_g, path=_path: c.path == path and ER.options(c)["gemm"] == g
for _a in (0, 1, 3):
    for _path in ("image", "text"):
        BRANCHES[f"{_path}, attn {_a}"] = lambda c, p, a=_a, path=_path: c.path == path and ER.options(c)["attn"] == a
for _path in ("image", "text"):
    for _fold in (False, True):
        BRANCHES[f"{_path}, gelu_exact, folded {_fold}"] = lambda c, p, path=_path, fold=_fold: c.path == path and ER.options(c)["gelu_exact"] == 1 and \
            any(r["hook"] == "lnfold" for r in p) == fold
    BRANCHES[f"{_path}, ln_fold 0 where the shape folds"] = lambda c, p, path=_path: c.path == path and ER.options(c)["ln_fold"] == 0 and \
        any(r["hook"] == "gemm" and r["epi"] == ER.EPI_BIAS and r["M"] >= 256 and r["K"] % 256 == 0 and
            ER.can_fold(dict(ER.options(c), ln_fold=1), r["M"], r["K"]) for r in p)
BRANCHES["fuse_im2col 0 where the GEMM would gather"] = lambda c, p: c.path == "image" and ER.options(c)["fuse_im2col"] == 0 and \
    any(r["hook"] == "im2col" and r["B"] * (r["R"] // 16) ** 2 >= 256 and not r["f32"] for r in p)


def test_cases_reach_every_branch():
    plans = {c.name: ER.plan(c) for c in ER.CASES}
    missing = [b for b, hits in BRANCHES.items() if not any(hits(c, plans[c.name]) for c in ER.CASES)]
    assert not missing, f"no case reaches: {missing}"
    # localisation: a geometry of the default options with more than two blocks in the tower it runs also appears with one and with two
    names = set(CASE_IDS)
    for base, one, two in (("small", "small1", "small2"),):
        for c in ER.CASES:
            if c.spec == base and not c.opts and c.path != "gen" and "raw" not in c.name and "chunks" not in c.name and "ensemble" not in c.name:
                for other in (one, two):
                    assert c.name.replace(f"_{base}_", f"_{other}_") in names, (c.name, other)
    for two, one in (("tiny", "tiny1"), ("b16x2", "b16x1"), ("head768", "head768x1")):
        assert any(c.spec == one for c in ER.CASES) and any(c.spec == two for c in ER.CASES)
    # no hook outside the library's (and the two copies, and the mutations' index write)
    hooks = {r["hook"] for p in plans.values() for r in p}
    assert hooks <= {"gemm", "gemm_patches", "gemm_strided", "lnfold", "layernorm", "attention", "attention_q", "attention_f32_varlen",
                     "attention_f32_long", "l2norm", "text_ensemble", "text_embed_ids", "text_add_pos", "gather_rows", "im2col", "fill_cls",
                     "agg_input", "agg_output"}, hooks


def test_every_mutation_runs_somewhere():
    hit = {m: [c.name for c in ER.CASES if m in ER.mutations_of(c)] for m in ER.MUTATIONS}
    assert all(hit.values()), [m for m, v in hit.items() if not v]
    # ... and "one normalisation more" on an output that is not normalised already, in both towers
    for path in ("image", "text"):
        ok = False
        for c in ER.CASES:
            if c.path == path:
                be = ER.Planner()
                ER.run(be, c, "norm_once_more")
                ok = ok or (be.hit and not be.rounding_only)
                assert ("norm_once_more" in ER.mutations_of(c)) == (be.hit and not be.rounding_only)
        assert ok, path


@pytest.mark.parametrize("name", CASE_IDS)
def test_every_mutation_changes_the_result(name):
    """In fp64 a wiring slip moves the result by far more than the 1e-9 two fp64 evaluations of the same wiring may differ by.  One
    normalisation more on rows that are normalised already is the identity (mutations_of leaves it out): there the result must NOT move."""
    case, t0 = ER.BY_NAME[name], time.time()
    want, be = _replay(case, torch.float64)
    assert not be.hit
    muts, same = ER.mutations_of(case), ER.mutations_of(case, identities=True)
    assert muts, name
    for m in muts + same:
        got, bm = _replay(case, torch.float64, m)
        assert bm.hit and bm.rounding_only == (m in same)
        d = _distance(got, [w.double() for w in want])
        if m in same:
            assert d <= 1e-9, f"{name}, {m}: {d:.3e}"
        else:
            assert d > 1e-9, f"{name}: '{ER.MUTATIONS[m]}' leaves the result where it was ({d:.3e})"
    print(f"\n{name}: {len(muts)} mutations, {time.time() - t0:.2f} s")
