"""Exemplar classes beyond 126 images on the HIP path: option "agg_max_len" (include/ovmr_hip.h) lifts the 128-row limit of the fp32
aggregator attention, a chunk whose longest class has more than 128 rows runs attn_f32_long (tests/test_hip_agg_long_kernels.py) for
all its classes.  The ragged call's contract holds at any length: class c equals the uniform call on class c alone, whatever shares
the call and wherever the chunk boundaries fall; and a class of at most 126 shots gets the bits an engine that never heard of the
option gives it.  The engines are built in this file: those of the other modules keep the option's default.
Needs an MI355X: `pytest -m gpu`.
"""
import numpy as np
import pytest
import torch

from conftest import COS_TOL, assert_cosine
from ovmr_amd import synth

pytestmark = pytest.mark.gpu
SEED = 11
SHOTS = [1, 16, 126, 127, 3, 300, 64, 255]       # 128 rows (the small kernel's limit), one more, two and a half key blocks, 257 rows


@pytest.fixture(scope="module")
def O():
    from oracle import ovmr_oracle
    return ovmr_oracle


def _engine(name, n_ctx=2, reserve=(64, 64, 256), agg_max_len=None, after_finalize=False):
    """test_hip_ragged._engine, with the option set before finalize (so that the aggregator's workspace holds one class of that
    length) or after it."""
    from ovmr_amd import modules
    spec = synth.SPECS[name]
    sd = {k: torch.from_numpy(v) for k, v in synth.clip_state_dict(spec, SEED, jitter=True).items()}
    e = modules.CLIPModel(sd, spec).engine(n_ctx)
    e.load_state_dict({}, {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, n_ctx, SEED, True).items()})
    e._pl_loaded = True
    if agg_max_len is not None and not after_finalize:
        e.set_option("agg_max_len", agg_max_len)
    e.finalize(*reserve)
    if agg_max_len is not None and after_finalize:
        e.set_option("agg_max_len", agg_max_len)
    return e


def _feats(spec, shots, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(sum(shots), spec.embed_dim, generator=g), dim=-1).half()


def _split(feats, shots):
    return list(torch.split(feats, list(shots)))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _oracle_tokens(O, rows, n_ctx=2, name="small"):
    """The reference's aggregator over cat([cls_token, feats_c]) at num_ins = len(rows) (trainers/mm_classifier_one_prompt.py:167-169)."""
    spec = synth.SPECS[name]
    pl = {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, n_ctx, SEED, True).items()}
    with torch.no_grad():
        x = torch.cat([pl["cls_token"], rows.float().cpu()], dim=0).unsqueeze(0)
        return O.transformer(x, pl, "aggregator.resblocks.", spec.embed_dim // 64, None)[0, :n_ctx]


@pytest.fixture(scope="module")
def long_case():
    """The `small` engine at agg_max_len = 600, the packed features of SHOTS and the ragged call's tokens: computed once, shared,
    left unchanged."""
    e = _engine("small", agg_max_len=600)
    feats = _feats(synth.SPECS["small"], SHOTS, 21).cuda()
    tokens = e.generate_tokens_ragged(feats, SHOTS)
    torch.cuda.synchronize()
    return e, feats, tokens


def test_option_values(O, long_case):
    """128 .. 4096 and nothing else; at 600 a 129-row and a 302-row class meet the oracle's aggregator at the tolerances of
    test_config_c4_sixty_four_shots, and 601 rows are refused with the option's value in the message and the tokens untouched."""
    from ovmr_amd.runtime import OvmrError, _ptr, _stream
    spec = synth.SPECS["small"]
    D = spec.embed_dim
    fresh = _engine("small")
    for bad in (100, 5000):
        with pytest.raises(OvmrError):
            fresh.set_option("agg_max_len", bad)
    assert "agg_max_len" not in fresh._options
    with pytest.raises(OvmrError, match="exceeds 128"):                     # a refused value left the option as it was
        fresh.generate_tokens(torch.zeros(1, 127, D, dtype=torch.float16))
    e = long_case[0]
    for Cb, S in ((2, 127), (1, 300)):
        feats = _feats(spec, [S] * Cb, 500 + S).view(Cb, S, D)
        tokens = e.generate_tokens(feats).cpu()
        assert tokens.shape == (Cb, 2, D)
        for c in range(Cb):
            np.testing.assert_allclose(tokens[c].numpy(), _oracle_tokens(O, feats[c]).numpy(), atol=5e-4, rtol=1e-3, err_msg=f"S = {S}, class {c}")
    feats = torch.zeros(1, 599, D, dtype=torch.float16, device="cuda")
    out = torch.empty((1, 2, D), device="cuda")
    out.view(torch.int32).fill_(0x5A5A5A5A)
    rc = e.lib.ovmr_generate_tokens(e.h, _ptr(feats), 1, 599, _ptr(out), _stream())
    torch.cuda.synchronize()
    assert rc == -2 and "exceeds 600" in e.lib.ovmr_last_error(e.h).decode()
    assert bool((out.view(torch.int32) == 0x5A5A5A5A).all()), "a refused call wrote tokens"


def test_ragged_mixed_chunk(O, long_case):
    """One ragged call over SHOTS (one chunk: 808 rows, the longest class 302, so every class goes through attn_f32_long).  Every class
    is bit-equal to the uniform call on it alone (a class of up to 126 shots alone runs attn_f32_small); every class of at most 126
    shots is also bit-equal to what a default engine, option never set, returns for it alone: the short classes of a mixed chunk did
    not move; and every class meets the oracle."""
    e, feats, tokens = long_case
    default = _engine("small")
    assert "agg_max_len" not in default._options
    assert tokens.shape == (len(SHOTS), 2, synth.SPECS["small"].embed_dim) and tokens.dtype == torch.float32
    for c, rows in enumerate(_split(feats, SHOTS)):
        alone = e.generate_tokens(rows.unsqueeze(0).contiguous())
        assert torch.equal(_bits(tokens[c]), _bits(alone[0])), f"class {c} ({SHOTS[c]} shots) != the uniform call on it alone"
        if SHOTS[c] <= 126:
            old = default.generate_tokens(rows.unsqueeze(0).contiguous())
            assert torch.equal(_bits(tokens[c]), _bits(old[0])), f"class {c} ({SHOTS[c]} shots) moved against a default engine"
        np.testing.assert_allclose(tokens[c].cpu().numpy(), _oracle_tokens(O, rows).numpy(), atol=5e-4, rtol=1e-3, err_msg=f"class {c}")


def test_ragged_chunks_do_not_change_a_bit(long_case):
    """finalize(max_classes = 3) with the option set before it: the aggregator's capacity is max(3 * 34, 600) = 600 rows, so the call
    runs as [1, 16, 126, 127, 3, 300] (585 rows) and [64, 255] (323 rows), the boundary behind the longest class.  Bit-equal to the
    one-chunk call.  (test_option_after_finalize runs the same call at 34 rows: every class but the first two a chunk of its own, the
    short ones through attn_f32_small.)"""
    e, feats, tokens = long_case
    e3 = _engine("small", reserve=(64, 64, 3), agg_max_len=600)
    got = e3.generate_tokens_ragged(feats, SHOTS)
    assert torch.equal(_bits(got), _bits(tokens))


def test_option_after_finalize(long_case):
    """The option raised AFTER finalize, on an engine finalised for one class (34 aggregator rows): a class needs a chunk of its own
    and that chunk has to fit the workspace finalize allocated.  The arena is the largest of the four passes, and on every model size
    here the head's logits buffers (192 MiB) are far larger than 4096 aggregator rows (38 MiB at embed_dim 256), so the "do not fit the
    workspace" refusal of generate_tokens cannot be reached from a test; what CAN be checked is that such an engine then runs the class
    and gives the bits of an engine that had the option before finalize."""
    e, feats, tokens = long_case
    late = _engine("small", reserve=(64, 64, 1), agg_max_len=4096, after_finalize=True)
    rows = _split(feats, SHOTS)[5]                                          # the 300-shot class
    got = late.generate_tokens(rows.unsqueeze(0).contiguous())
    assert torch.equal(_bits(got[0]), _bits(tokens[5]))
    got = late.generate_tokens_ragged(feats, SHOTS)                         # one class per chunk but the first two
    assert torch.equal(_bits(got), _bits(tokens))


def test_all_equal_shots_equal_the_uniform_call(long_case):
    e = long_case[0]
    feats = _feats(synth.SPECS["small"], [130] * 3, 230).cuda()
    assert torch.equal(_bits(e.generate_tokens_ragged(feats, [130] * 3)), _bits(e.generate_tokens(feats.view(3, 130, -1))))


# ---- forward_prompt on `tiny` (32-px images: cheap on the CPU oracle) -----------------------------------------------------------------
IMG_SEED, TOK_SEED = 2, 4


def _tiny_job(shots):
    spec = synth.SPECS["tiny"]
    labels = np.repeat(np.arange(len(shots)), shots)
    img = torch.from_numpy(synth.images(len(labels), spec.image_resolution, IMG_SEED, labels, 0.9))
    tok = torch.from_numpy(synth.class_token_ids(len(shots), seed=TOK_SEED))
    pl = {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, 2, SEED, True).items()}
    return spec, labels, img, tok, pl


def _tiny_model(tok, pl, num_shots, batch):
    from ovmr_amd import modules
    spec = synth.SPECS["tiny"]
    sd = {k: torch.from_numpy(v) for k, v in synth.clip_state_dict(spec, SEED, jitter=True).items()}
    cfg = modules.make_cfg(n_ctx=2, num_shots=num_shots, output_dir="", test_batch_size=batch, size=spec.image_resolution)
    return modules.CustomCLIP(cfg, tok, modules.CLIPModel(sd, spec), prompt_learner_state=pl, reserve=(64, 64, 256))


def _check(O, model, img, labels, shots, tok, pl, what):
    from test_hip_parity import _oracle_sd
    from test_hip_ragged import _oracle_ragged
    r = _oracle_ragged(O, img, labels, dict(enumerate(shots)), tok, _oracle_sd(O, "tiny"), pl)
    assert_cosine(model.mm_classifier.float().cpu().numpy(), r["mm"].numpy(), COS_TOL, f"{what}: mm")
    assert_cosine(model.visual_classifer.float().cpu().numpy(), r["v"].numpy(), COS_TOL, f"{what}: vision")
    assert_cosine(model.visual_tokens.float().cpu().numpy(), r["tokens"].float().numpy(), COS_TOL, f"{what}: visual_tokens")


def test_forward_prompt_130_shots_uniform(O):
    """CustomCLIP with NUM_SHOTS = 130, three classes, the uniform layout: it sets agg_max_len = 132 on its engine before finalising,
    and mm_classifier, vision_classifier and the visual tokens meet the oracle at the BASELINE bar (1 - cos <= 1e-3).  A CustomCLIP
    with NUM_SHOTS = 16 sets nothing."""
    from ovmr_amd.data import ResidentEvalSet
    shots = [130] * 3
    spec, labels, img, tok, pl = _tiny_job(shots)
    model = _tiny_model(tok, pl, 130, 260)
    assert model.engine._options.get("agg_max_len") == 132
    model.forward_prompt(ResidentEvalSet(img, torch.arange(3), 130, 2))
    _check(O, model, img, labels, shots, tok, pl, "130 shots")
    plain = _tiny_model(tok, pl, 16, 64)
    assert "agg_max_len" not in plain.engine._options


def test_forward_prompt_ragged_long_classes(O):
    """Ragged shots [130, 4, 200] under NUM_SHOTS = 200, whole classes per loader batch of at most 200 rows."""
    from ovmr_amd.data import ResidentRaggedSet
    shots = [130, 4, 200]
    spec, labels, img, tok, pl = _tiny_job(shots)
    model = _tiny_model(tok, pl, 200, 200)
    assert model.engine._options.get("agg_max_len") == 202
    loader = ResidentRaggedSet(img, labels, 200, num_classes=3)
    assert loader.shots.tolist() == shots and len(loader) == 2
    model.forward_prompt(loader)
    assert model.eval_row_labels.cpu().tolist() == labels.tolist()
    _check(O, model, img, labels, shots, tok, pl, "ragged [130, 4, 200]")
