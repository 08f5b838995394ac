"""The layouts the Python boundary repairs, on the GPU (tests/boundary_cases.py states them; tests/test_boundary_cpu.py proves without a GPU
that a mis-shaped call cannot reach the library -- no violation is run here).  One `tiny` engine with synth weights:

  every accepted call that is not in the plain layout -- numpy and host input, transposed / permuted views, channels-last images, slices with
  a storage offset, expanded rows, fp64 / uint8 images, int32 ids and labels, empty batches, a caller's `out=` -- gives the BITS of the same
  call on fresh contiguous operands of the target dtype on the device;
  where `out=` is a slice of a larger buffer, every byte outside the slice keeps the sentinel it was filled with;
  the library is reached once, and what it is handed covers what the header derives from the scalars of that call (boundary_cases.check_call,
  here against the real addresses)."""
import pytest
import torch

import boundary_cases as bc
from ovmr_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 11


def _new_engine():
    from ovmr_amd.runtime import Engine
    e = Engine(bc.SPEC, bc.N_CTX, DEV)
    e.load_state_dict({k: torch.from_numpy(v) for k, v in synth.clip_state_dict(bc.SPEC, SEED, jitter=True).items()},
                      {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(bc.SPEC, bc.N_CTX, SEED, True).items()})
    e.finalize(8, 16, 8)
    return e


@pytest.fixture(scope="module")
def engine():
    return _new_engine()


@pytest.fixture
def seam(engine, monkeypatch):
    """The real library behind a recorder, and the tensors behind the addresses it is handed."""
    from ovmr_amd import runtime
    held, real_ptr, lib = {}, runtime._ptr, runtime.load_library()
    rec = bc.Recorder(forward=lib)

    def ptr(t):
        if t is not None:
            held[t.data_ptr()] = t
        return real_ptr(t)

    monkeypatch.setattr(runtime, "_ptr", ptr)
    monkeypatch.setattr(runtime, "load_library", lambda path=None: rec)
    monkeypatch.setattr(engine, "lib", rec)
    return rec, held


def _bits(t):
    """A result as integers: fp16 as int16, fp32 as int32 (tests/*_exact.py compare the same way)."""
    t = t.detach().contiguous()
    return t.view({torch.float16: torch.int16, torch.float32: torch.int32}.get(t.dtype, t.dtype)).cpu()


def _results(r):
    return [_bits(x) for x in (r if isinstance(r, (tuple, list)) else (r,))]


LAID = [c for c in bc.ACCEPTED if c.name != "plain" and c.wrapper != "set_weight"]


@pytest.mark.parametrize("case", LAID, ids=[bc.case_id(c) for c in LAID])
def test_layout_gives_the_bits_of_the_plain_call(case, engine, seam):
    rec, held = seam
    ops = case.build(DEV)
    want = _results(bc.CALLS[case.wrapper](engine, bc.plain_of(case.wrapper, ops, DEV)))
    rec.calls.clear()
    held.clear()
    got = _results(bc.CALLS[case.wrapper](engine, ops))
    torch.cuda.synchronize()
    launches = rec.launches()
    assert [n for n, _ in launches] == [bc.ENTRY[case.wrapper]]
    problems = bc.check_call(*launches[0], held)
    assert not problems, "\n".join(problems)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        assert torch.equal(g, w), f"result {k}: {int((g != w).sum())} of {g.numel()} elements differ from the plain call"
    out = ops.get("out")
    if out is not None:                                   # a caller's buffer: written where it says, and nowhere else
        whole = out.whole                                 # the buffer boundary_cases filled with the sentinel, as uint8
        assert whole.dtype == torch.uint8 and whole.numel() >= out.numel() * out.element_size()
        if out.numel():
            assert not torch.equal(_bits(out), _bits(_sentinel_like(out))), "the call wrote nothing"
        out.copy_(_sentinel_like(out))
        torch.cuda.synchronize()
        assert bool((whole == bc.SENTINEL).all()), f"{int((whole != bc.SENTINEL).sum())} bytes outside `out` lost the sentinel"


def _sentinel_like(out):
    item = out.element_size()
    return torch.full((item,), bc.SENTINEL, dtype=torch.uint8, device=out.device).view(out.dtype).expand(out.shape)


def test_set_weight_layouts_give_the_same_model():
    """set_weight has no output of its own: the text projection in every accepted layout, then the features it gives."""
    e = _new_engine()
    ids = torch.from_numpy(synth.class_token_ids(3)).to(DEV)

    def feats(ops):
        bc.CALLS["set_weight"](e, ops)
        e.finalize(8, 16, 8)
        return _bits(e.encode_text_ids(ids))

    base = feats(bc.BASE["set_weight"](DEV))
    other = feats(dict(bc.BASE["set_weight"](DEV), tensor=bc.BASE["set_weight"](DEV)["tensor"] * 2))
    assert not torch.equal(base, other)                   # (the weight is read: the comparison below means something)
    for case in bc.ACCEPTED:
        if case.wrapper == "set_weight" and case.name != "plain":
            ops = case.build(DEV)
            want = feats(bc.plain_of("set_weight", ops, DEV))
            assert torch.equal(feats(ops), want), bc.case_id(case)
            if "fp16" not in case.name:
                assert torch.equal(want, base), bc.case_id(case)
    torch.cuda.synchronize()
