"""The Python boundary without a GPU and without the library (tests/boundary_cases.py states the contract): a real runtime.Engine, built
with object.__new__, on a recording stand-in for libovmr_hip.so.

  violations   every mis-shaped call raises ValueError naming the wrapper, the argument, what it must be and what it is -- and the
               recorder has seen NO call, nothing was copied to the device (Engine._dev) and no stream was asked for
  accepted     every well-formed call, in every layout the wrappers repair, reaches the library exactly once; each tensor behind an
               address is contiguous, of the header's dtype, and covers what the header derives from the scalars ACTUALLY passed
  controls     with the checks bypassed the two violations that were reproduced on the parent commit reach the recorder, and the header's
               formula finds the shortfall; every entry point of runtime.SIGNATURES is classified
  modules.py   the module API (CustomCLIP.forward / forward_batches / predict_topk, the split forward, CLIPModel, TextEncoder, PromptLearner,
               ZeroshotCLIP, trainer.ZeroshotCLIP.model_inference) refuses the same way, before it stages a batch or touches a side stream"""
import ctypes
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import boundary_cases as bc
from ovmr_amd import loader, modules, runtime, synth, trainer

WHERE = {"eval_counts": "Classification.process"}          # the name a refusal carries, where it is not the wrapper's own


class _Stream:
    cuda_stream = 0

    def __init__(self, log):
        log.append("stream")

    def synchronize(self):
        pass


@pytest.fixture
def stub(monkeypatch):
    """(engine, recorder, address -> tensor, log of copies and stream requests): the Engine of ovmr_amd.runtime on a recording library."""
    rec, held, log = bc.Recorder(), {}, []
    real_ptr, real_dev = runtime._ptr, runtime.Engine._dev

    def ptr(t):
        if t is not None:
            held[t.data_ptr()] = t
        return real_ptr(t)

    def dev(self, t, dtype=None):
        log.append("copy")
        return real_dev(self, t, dtype)

    monkeypatch.setattr(runtime, "_ptr", ptr)
    monkeypatch.setattr(runtime.Engine, "_dev", dev)
    monkeypatch.setattr(runtime, "_stream", lambda: log.append("stream"))
    monkeypatch.setattr(runtime, "load_library", lambda path=None: rec)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _Stream(log))
    e = object.__new__(runtime.Engine)
    e.lib, e.spec, e.n_ctx, e.device, e.h, e.finalized = rec, bc.SPEC, bc.N_CTX, torch.device("cpu"), ctypes.c_void_p(1), True
    e._options, e._weights_version = {}, 0
    yield SimpleNamespace(e=e, rec=rec, held=held, log=log)
    e.h = None                                             # (nothing for __del__ to destroy)


def _ids(cases):
    return [bc.case_id(c) for c in cases]


# ------------------------------------------------------------------------------------------------------------------------ violations
@pytest.mark.parametrize("case", bc.VIOLATIONS, ids=_ids(bc.VIOLATIONS))
def test_violation_is_refused_before_anything_launches(case, stub, monkeypatch):
    if bc.NEEDS_DEVICE(case):                              # a device-only wrapper: host tensors stand for device tensors, every other check stays
        monkeypatch.setattr(runtime, "_same_device", lambda a, b: True, raising=False)
    ops = case.build("cpu")
    with pytest.raises(ValueError) as err:
        bc.CALLS[case.wrapper](stub.e, ops)
    msg = str(err.value)
    assert WHERE.get(case.wrapper, case.wrapper) in msg, msg
    assert re.search(rf"(?<![\w]){re.escape(case.arg)}(?![\w])", msg), f"the message does not name `{case.arg}`: {msg}"
    assert "must be" in msg and "got" in msg, msg
    x = ops.get(case.arg)
    if isinstance(x, (torch.Tensor, np.ndarray)):          # what was got: the offending operand's shape, dtype, strides, device or values
        got = [str(list(x.shape)), str(x.dtype), "values from", "a numpy array"]
        if isinstance(x, torch.Tensor):
            got += [str(tuple(x.stride())), f"on {x.device}"]
        assert any(g in msg.split("got", 1)[1] for g in got), msg
    assert stub.rec.calls == [], f"the library was reached: {[n for n, _ in stub.rec.calls]}"
    assert stub.log == [], f"a refused call must not copy or ask for a stream: {stub.log}"


def test_violation_table_covers_what_the_issue_lists():
    """One line per kind of violation the contract names, by wrapper and argument (the table may hold more)."""
    have = {(c.wrapper, c.arg) for c in bc.VIOLATIONS}
    for pair in [("encode_image", "image"), ("encode_image", "out"), ("encode_text_ids", "ids"), ("encode_text_embedded", "prompts"),
                 ("encode_text_embedded", "index"), ("encode_text_groups", "ids"), ("encode_text_groups", "prompts"),
                 ("encode_text_groups", "index"), ("encode_text_ensemble", "ids"), ("encode_text_ensemble", "seq_lens"), ("embed_tokens", "ids"),
                 ("generate_tokens", "feats"), ("generate_tokens_ragged", "feats"), ("assemble_prompts", "base"),
                 ("assemble_prompts", "tokens"), ("assemble_prompts", "labels"), ("xval_counts", "labels"), ("xval_counts", "clf"),
                 ("xval_counts", "tp"), ("xval_counts", "n_pred"), ("fusion_weights", "counts"), ("fused_logits", "w"), ("fused_logits", "v"),
                 ("fused_logits_all", "w"), ("fused_logits_all", "out"), ("zeroshot_logits", "text_feats"), ("zeroshot_logits", "out"),
                 ("pack_rows", "tokens"), ("unpack_rows", "gathered"), ("preprocess_u8", "u8"), ("preprocess_u8", "out")]:
        assert pair in have, pair
    names = " | ".join(bc.case_id(c) for c in bc.VIOLATIONS)
    for word in ("resolution 8", "resolution 40", "one channel", "three dimensions", "ids [3, 5]", "width 64", "index longer", "a row less",
                 "w [C, 2]", "counts [3, 2, C - 1]", "tp shorter", "tp int64", "tokens of 3 rows", "a column short", "out fp32",
                 "on another device", "out strided", "not square", "side 36", "seq_lens", "vocab_size (host)", "beyond base's rows (host)"):
        assert word in names, word


# -------------------------------------------------------------------------------------------------------------------------- accepted
HOST_RUNNABLE = [c for c in bc.ACCEPTED if c.wrapper not in bc.DEVICE_ONLY]


@pytest.mark.parametrize("case", HOST_RUNNABLE, ids=_ids(HOST_RUNNABLE))
def test_accepted_call_hands_over_what_the_header_asks(case, stub):
    ops = case.build("cpu")
    bc.CALLS[case.wrapper](stub.e, ops)
    launches = stub.rec.launches()
    assert [n for n, _ in launches] == [bc.ENTRY[case.wrapper]]
    problems = bc.check_call(*launches[0], stub.held)
    assert not problems, "\n".join(problems)


def test_accepted_out_is_what_the_library_writes(stub):
    """A caller's `out=` is the tensor whose address goes to the library, and the tensor returned."""
    for case in HOST_RUNNABLE:
        ops = case.build("cpu")
        if "out" in ops:
            stub.rec.calls.clear()
            res = bc.CALLS[case.wrapper](stub.e, ops)
            (_, args), = stub.rec.launches()
            assert res is ops["out"] and (res.numel() == 0 or any(isinstance(a, ctypes.c_void_p) and a.value == ops["out"].data_ptr() for a in args)), bc.case_id(case)


# -------------------------------------------------------------------------------------------------------------------------- controls
@pytest.mark.parametrize("name, entry, short", [("encode_image: resolution 8", "ovmr_encode_image", "image covers 384 elements, the call's scalars need 6144"),
                                                ("encode_text_ids: ids [3, 5]", "ovmr_encode_text_ids", "ids covers 15 elements, the call's scalars need 231")])
def test_control_without_the_checks_the_launch_is_seen(name, entry, short, stub, monkeypatch):
    """The recorder would have seen what the checks refuse: with _want bypassed (the parent commit's behaviour) the call goes through, and
    the header's formula, applied to the scalars that were passed, finds the buffer too short."""
    monkeypatch.setattr(runtime, "_want", lambda *a, **k: None, raising=False)
    case, = [c for c in bc.VIOLATIONS if bc.case_id(c) == name]
    bc.CALLS[case.wrapper](stub.e, case.build("cpu"))
    (got, args), = stub.rec.launches()
    assert got == entry
    assert any(short in p for p in bc.check_call(got, args, stub.held)), bc.check_call(got, args, stub.held)


def test_control_every_entry_point_is_classified():
    names = set(runtime.SIGNATURES)
    assert not set(bc.ABI) & bc.EXEMPT
    assert names == set(bc.ABI) | bc.EXEMPT, f"unclassified: {sorted(names - set(bc.ABI) - bc.EXEMPT)}, gone: {sorted((set(bc.ABI) | bc.EXEMPT) - names)}"
    assert set(bc.ENTRY.values()) == set(bc.ABI) and set(bc.CALLS) == set(bc.BASE) == set(bc.ENTRY)
    for wrapper, entry in bc.ENTRY.items():
        assert any(c.wrapper == wrapper for c in bc.ACCEPTED) and any(c.wrapper == wrapper for c in bc.VIOLATIONS), entry
    for entry in bc.ABI:                                   # an entry point with a formula takes at least one address
        assert ctypes.c_void_p in runtime.SIGNATURES[entry][1] or any(a is not ctypes.c_int for a in runtime.SIGNATURES[entry][1])


def test_control_extent_and_recorder():
    big = torch.zeros(4, 7, 5)
    assert bc.extent(big) == 140 and bc.extent(big[:, 2:5]) == 3 * 35 + 15 and bc.extent(big[1:1]) == 0 and bc.extent(big.permute(2, 1, 0)[:2]) == 1 + 1 + 6 * 5 + 3 * 35
    rec = bc.Recorder()
    assert rec.ovmr_head_plan(None, 1, 2) == 0 and rec.ovmr_encode_image(None) == 0 and [n for n, _ in rec.launches()] == ["ovmr_encode_image"]
    t = torch.zeros(3, 5)
    args = (None, ctypes.c_void_p(t.data_ptr()), 3, None, 5, ctypes.c_void_p(t.data_ptr()), None)      # zeroshot_logits claiming 3 x 128 features
    assert len(bc.check_call("ovmr_zeroshot_logits", args, {t.data_ptr(): t})) >= 3                       # dtype, feats and text too short


# ------------------------------------------------------------------------------------------------------------------------ modules.py
C_MOD = 4


@pytest.fixture
def model(stub, monkeypatch):
    """modules.CustomCLIP and modules.ZeroshotCLIP, built by their own constructors on the stub engine."""
    def no_side_stream(*a, **k):
        raise AssertionError("a side stream was made for a batch that must be refused")
    monkeypatch.setattr(torch.cuda, "Stream", no_side_stream)
    clip = object.__new__(modules.CLIPModel)
    clip._sd, clip.spec, clip.device, clip.dtype = {}, bc.SPEC, torch.device("cpu"), torch.float16
    clip.logit_scale, clip.context_length, clip.vocab_size, clip._engines = torch.tensor(4.6), bc.SPEC.context_length, bc.SPEC.vocab_size, {bc.N_CTX: stub.e}
    pl = {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(bc.SPEC, bc.N_CTX, 3).items()}
    tok = torch.from_numpy(synth.class_token_ids(C_MOD))
    m = modules.CustomCLIP(modules.make_cfg(n_ctx=bc.N_CTX, num_shots=4), tok, clip, prompt_learner_state=pl, reserve=(8, 8, 8))
    m.mm_classifier = m.visual_classifer = torch.zeros(C_MOD, bc.E, dtype=torch.float16)
    m.fusion_weight = torch.zeros(C_MOD, 3)
    zs = modules.ZeroshotCLIP(clip, tok, reserve=(8, 8, 8))
    stub.rec.calls.clear()
    stub.log.clear()
    return SimpleNamespace(m=m, zs=zs, clip=clip, tok=tok)


def _refused(stub, call, arg):
    with pytest.raises(ValueError, match=rf"\b{arg} must be .* got "):
        call()
    assert stub.rec.launches() == [] and "copy" not in stub.log, (stub.rec.calls, stub.log)


@pytest.mark.parametrize("image", [torch.zeros(4, 3, 8, 8), torch.zeros(4, 3, 40, 40), torch.zeros(4, 32, 32, 3), torch.zeros(3, 32, 32),
                                   np.zeros((4, 1, 32, 32), dtype=np.float32)], ids=["resolution 8", "resolution 40", "channels last", "3-d", "1 channel"])
def test_modules_refuse_a_malformed_image(image, stub, model):
    m, zs = model.m, model.zs
    _refused(stub, lambda: m.forward(image), "image")
    _refused(stub, lambda: m(image), "image")
    _refused(stub, lambda: list(m.forward_batches([image])), "image")
    _refused(stub, lambda: list(m.forward_batches([image], overlap=True)), "image")
    _refused(stub, lambda: m.predict_topk(image, 2), "image")
    _refused(stub, lambda: list(m.predict_topk_batches([image], 2)), "image")
    _refused(stub, lambda: model.clip.encode_image(image), "image")
    _refused(stub, lambda: m.image_encoder(image), "image")
    _refused(stub, lambda: zs.model_inference(image), "image")
    _refused(stub, lambda: list(zs.inference_batches([image], overlap=True)), "image")
    _refused(stub, lambda: zs.predict_topk(image, 2), "image")
    t = object.__new__(trainer.ZeroshotCLIP)
    t.model = zs
    _refused(stub, lambda: t.model_inference(image), "image")
    assert not hasattr(m, "_overlap_streams") and not hasattr(zs, "_overlap_streams")
    m.SPLIT_MIN_HALF = 1                                   # the split forward: two halves on two handles -- refused before the side stream exists
    if image.ndim == 4:
        assert m.SPLIT_FORWARD and 2 <= image.shape[0] <= m._split_cap() and m._split_keeps_bits(image.shape[0])
        stub.rec.calls.clear()
    _refused(stub, lambda: m.forward(image), "image")
    _refused(stub, lambda: m._forward_split(image), "image")
    assert not hasattr(m, "_split_stream") and not hasattr(m, "_twin_engines")


def test_modules_refuse_malformed_text_and_features(stub, model):
    m, tok = model.m, model.tok
    _refused(stub, lambda: model.clip.encode_text(tok[:, :5]), "ids")
    _refused(stub, lambda: modules.ZeroshotCLIP(model.clip, tok[:, :5]), "ids")
    _refused(stub, lambda: modules.ZeroshotCLIP2(model.clip, torch.stack([tok, tok])[:, :, :5]), "ids")
    _refused(stub, lambda: m.prompt_learner.encode_zero_shot(tok[:, :76]), "ids")
    prompts, eos = torch.zeros(C_MOD, bc.CTX, bc.W, dtype=torch.float16), torch.full((C_MOD,), 5)
    _refused(stub, lambda: m.text_encoder(prompts[:, :5], eos), "prompts")
    _refused(stub, lambda: m.text_encoder(prompts[:, :, :64], eos), "prompts")
    _refused(stub, lambda: m.text_encoder(prompts, eos[:3]), "index")
    feats, label, lens = torch.zeros(3, 4, bc.E, dtype=torch.float16), torch.tensor([2, 0, 1]), torch.tensor([5, 4, 6])
    _refused(stub, lambda: m.prompt_learner(feats[:, :, :64], label, lens), "feats")
    _refused(stub, lambda: m.prompt_learner(feats.flatten(0, 1)[:, :64], label, lens, shots=[4, 4, 4]), "feats")
    _refused(stub, lambda: m.get_mm_v_feats([prompts], eos, [prompts[:, :5]], eos), "prompts")
    # ... the generator ran, then a label that is no row of the class prompts: refused by assemble_prompts, on the host
    with pytest.raises(ValueError, match=r"assemble_prompts: labels must be rows of base in \[0, 4\), got values from 0 to 4"):
        m.prompt_learner(feats, torch.tensor([4, 0, 1]), lens)
    assert [n for n, _ in stub.rec.launches()] == ["ovmr_generate_tokens"]


def test_modules_well_formed_calls_still_go_through(stub, model):
    m, zs = model.m, model.zs
    image = torch.zeros(4, 3, bc.R, bc.R)
    out = m.forward(image)
    assert out.shape == (4, C_MOD) and [n for n, _ in stub.rec.launches()] == ["ovmr_encode_image", "ovmr_fused_logits"]
    for name, args in stub.rec.launches():
        assert not bc.check_call(name, args, stub.held)
    stub.rec.calls.clear()
    assert zs.model_inference(image.half().numpy()).shape == (4, C_MOD)
    assert [n for n, _ in stub.rec.launches()] == ["ovmr_encode_image", "ovmr_zeroshot_logits"]
    stub.rec.calls.clear()
    mm, mm_lens, v, v_lens, tokens = m.prompt_learner(torch.zeros(3, 4, bc.E), torch.tensor([2, 0, 3]), torch.tensor([5, 4, 6]))
    assert [n for n, _ in stub.rec.launches()] == ["ovmr_generate_tokens", "ovmr_assemble_prompts", "ovmr_assemble_prompts"]
    for name, args in stub.rec.launches():
        assert not bc.check_call(name, args, stub.held)
