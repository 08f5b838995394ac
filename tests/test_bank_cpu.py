"""The reference bank and the vocabulary edits without a GPU: the Python layer of ovmr_amd.modules (save_bank / load_bank, add / replace /
remove_classes) on the CPU stand-in engine of tests/test_distributed_cpu.py, and the runner's flag refusals.  The contract is DESIGN.md
section 6 ("Editing a generated vocabulary"): round trip, old classes untouched, counters a function of the state, an aligned edit equals
the from-scratch job bit for bit, an unaligned one meets the 1 - cos <= 1e-3 bar."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import COS_TOL, assert_cosine
from ovmr_amd import bank, synth
from ovmr_amd.synth import EOT_ID, SOT_ID
from test_distributed_cpu import N_CTX, SEED
from test_ragged_cpu import RaggedClipModel, RaggedOracleEngine

CAP = 4                                       # DATASET.NUM_SHOTS of the ragged jobs: the most a class may bring
UNIFORM = 3                                   # DATASET.NUM_SHOTS = images per class of the uniform jobs
SPEC = synth.SPECS["tiny"]
TOK_A, TOK_DOT = (int(t) for t in synth.template_token_ids()[0, 1:3])
# class u of the pool: its name's token ids (1 to 4 of them; the long one, 6, is longer than every other) and how many exemplars it brings
# in the ragged jobs.  Classes 0-5 are the old vocabulary, 6 and 7 the added ones, 8 the class with the longer name.
NAME_IDS = [[11, 12], [13, 14, 15, 16], [17], [18, 19, 20], [21, 22, 23, 24], [25, 26], [27, 28, 29], [30], [31, 32, 33, 34, 35, 36]]
RAGGED = [3, 1, 4, 2, 4, 1, 2, 4, 3]
RECORDED = ("finalize", "embed_tokens", "encode_image", "encode_text_ids", "encode_text_groups", "generate_tokens", "generate_tokens_ragged",
            "assemble_prompts", "xval_counts", "fusion_weights", "fused_logits")


def _rows(classes):
    out = torch.zeros(len(classes), SPEC.context_length, dtype=torch.long)
    for r, u in enumerate(classes):
        ids = [SOT_ID, TOK_A] + NAME_IDS[u] + [TOK_DOT, EOT_ID]
        out[r, :len(ids)] = torch.tensor(ids)
    return out


class BankEngine(RaggedOracleEngine):
    """The stand-in, with a record of every call the modules make (name, arguments of finalize)."""

    def __init__(self, spec, n_ctx, clip_seed):
        super().__init__(spec, n_ctx)
        if clip_seed != SEED:
            self.sd = self.O.convert_weights(self.O.to_torch(synth.clip_state_dict(spec, clip_seed, jitter=True)), "fp16")
        self.calls = []


def _recorded(name):
    def call(self, *a, **kw):
        self.calls.append((name, a if name == "finalize" else None))
        return getattr(RaggedOracleEngine, name)(self, *a, **kw)
    return call


for _name in RECORDED:
    setattr(BankEngine, _name, _recorded(_name))


_CLIP_STATE = {}                              # seed -> the CLIP state dict the stand-in's weights come from (generated once)


class BankClipModel(RaggedClipModel):
    def __init__(self, spec, clip_seed=SEED):
        super().__init__(spec)
        self.clip_seed = clip_seed

    def engine(self, n_ctx):
        if n_ctx not in self._e:
            self._e[n_ctx] = BankEngine(self.spec, n_ctx, self.clip_seed)
        return self._e[n_ctx]

    def state_dict(self):
        if self.clip_seed not in _CLIP_STATE:
            _CLIP_STATE[self.clip_seed] = {k: torch.from_numpy(v) for k, v in synth.clip_state_dict(self.spec, self.clip_seed, jitter=True).items()}
        return _CLIP_STATE[self.clip_seed]


class WordTokenizer:
    """encode(str) -> ids, one id per word ("a" and "." as the template's): enough of a tokenizer for class NAMES on the stand-in."""
    WORDS = {"a": TOK_A, ".": TOK_DOT}

    def encode(self, text):
        return [self.WORDS.get(w, 100 + sum(map(ord, w)) % 300) for w in text.replace(".", " .").split()]


_IMAGES = {}


def _images(u, version=0):
    """The exemplar images of class u (CAP of them; a ragged job takes the first RAGGED[u]); version 1: another set, for replace."""
    key = (u, version)
    if key not in _IMAGES:
        _IMAGES[key] = torch.from_numpy(synth.images(CAP, SPEC.image_resolution, 1000 + 50 * version + u, np.full(CAP, u), 0.6))
    return _IMAGES[key]


class OneClassPerBatch:
    """An eval-set loader over `classes` = [(u, version)], labelled 0 ... K - 1, ONE class per batch (so that every edit is aligned); ragged:
    the batches carry "shots" and the loader `.shots`, as cli.FolderLoader does; otherwise every class brings `uniform` images."""

    def __init__(self, classes, ragged, uniform=UNIFORM):
        self.classes, self.ragged, self.uniform = [c if isinstance(c, tuple) else (c, 0) for c in classes], ragged, uniform
        if ragged:
            self.shots = torch.tensor([RAGGED[u] for u, _ in self.classes], dtype=torch.int32)

    def __iter__(self):
        for k, (u, version) in enumerate(self.classes):
            n = RAGGED[u] if self.ragged else self.uniform
            batch = {"img": _images(u, version)[:n], "label": torch.full((n,), k, dtype=torch.long)}
            if self.ragged:
                batch["shots"] = torch.tensor([n], dtype=torch.long)
            yield batch


def _model(vocabulary, outdir="", tau=10.0, reserve=(8, 8, 8), clip_seed=SEED, pl_seed=SEED, tokenizer=None, ragged=True):
    from ovmr_amd import modules
    shots = CAP if ragged else UNIFORM
    cfg = modules.make_cfg(n_ctx=N_CTX, num_shots=shots, eval_tau=tau, output_dir=outdir, test_batch_size=shots)
    pl = {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(SPEC, N_CTX, pl_seed, True).items()}
    names = vocabulary if isinstance(vocabulary[0], str) else _rows(vocabulary)
    return modules.CustomCLIP(cfg, names, BankClipModel(SPEC, clip_seed), tokenizer=tokenizer, prompt_learner_state=pl, reserve=reserve,
                              stream_text=True)


def _scratch(classes, ragged, outdir="", **kw):
    """The from-scratch job on `classes` ([(u, version)] or [u]), exemplars walked in label order."""
    m = _model([c[0] if isinstance(c, tuple) else c for c in classes], outdir, ragged=ragged, **kw)
    m.forward_prompt(OneClassPerBatch(classes, ragged))
    return m


def _same_state(a, b, what):
    sa, sb = a.bank_state(), b.bank_state()
    assert list(sa) == list(bank.FIELDS) == list(sb)
    for k in bank.FIELDS:
        if isinstance(sa[k], torch.Tensor):
            assert sa[k].dtype == sb[k].dtype and torch.equal(sa[k], sb[k]), f"{what}: {k}"
        else:
            assert sa[k] == sb[k], f"{what}: {k}"


def _same_files(a, b, what):
    for name in ("mm_classifiers.pt", "visual_tokens.pt"):
        with open(os.path.join(a, name), "rb") as fa, open(os.path.join(b, name), "rb") as fb:
            assert fa.read() == fb.read(), f"{what}: {name}"


def _counters_are_a_function_of_the_state(m):
    """Contract point 3: a fresh _xval_fusion_weight on the model's own rows and classifiers gives its counters and weights, exactly."""
    counts, weights = m.xval_counts.clone(), m.fusion_weight.clone()
    fresh = m._xval_fusion_weight(torch.zeros(0, dtype=torch.long), m.mm_classifier, m.visual_classifer, m.zero_shot_classifier,
                                  float(m.cfg.EVAL_TAU))
    assert torch.equal(m.xval_counts, counts) and torch.equal(fresh, weights)
    R = m.eval_feat4cls.shape[0] if m.eval_row_labels is not None else m.eval_feat4cls.shape[0] * m.eval_feat4cls.shape[1]
    assert counts[:, 1].sum(-1).tolist() == [R, R, R]                       # every exemplar row voted once per classifier


def _vocabulary_is_consistent(m, C):
    pl = m.prompt_learner
    assert len(m.tokenized_prompts) == C == pl.num_class == pl.n_cls == len(pl.name_lens) and m.tokenized_prompts is pl.tokenized_prompts
    assert pl.eos_index.tolist() == pl.tokenized_prompts.argmax(-1).tolist() and pl.max_eos == int(pl.eos_index.max())
    assert pl.prompt_tokens.shape[0] == C and torch.equal(pl.prompt_tokens, m.engine.embed_tokens(pl.tokenized_prompts))
    assert m.inference_text_initialized.tolist() == [1] * C and m.zero_shot_classifier is pl.zero_shot_classifier
    for t in (m.mm_classifier, m.visual_classifer, m.zero_shot_classifier, m.visual_tokens, m.fusion_weight):
        assert t.shape[0] == C
    assert m.xval_counts.shape == (3, 2, C)


def _rows_of(m, keep):
    return [t[keep].clone() for t in (m.mm_classifier, m.visual_classifer, m.zero_shot_classifier, m.visual_tokens)]


@pytest.fixture(scope="module", autouse=True)
def _two_threads():
    threads = torch.get_num_threads()
    torch.set_num_threads(2)
    yield
    torch.set_num_threads(threads)


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """The 6-class jobs, uniform and ragged, with their files and banks: computed once, shared, never changed."""
    out = {}
    for ragged in (False, True):
        d = tmp_path_factory.mktemp("ragged" if ragged else "uniform")
        m = _scratch(range(6), ragged, str(d / "gen"))
        m.save_bank(str(d / "gen" / bank.BANK_FILE))
        out[ragged] = (m, d)
    return out


QUERY = torch.from_numpy(synth.images(5, SPEC.image_resolution, 777))


# ---- contract points 1 - 4 ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_round_trip(generated, ragged):
    """Point 1: save_bank -> load_bank on a fresh model (built for ANOTHER class list): every tensor, forward and both files are equal; the
    loaded model generates nothing."""
    m, d = generated[ragged]
    state = bank.read(str(d / "gen" / bank.BANK_FILE))
    assert state["format"] == bank.BANK_FORMAT and state["tau"] == 10.0 and state["num_shots_cap"] == (CAP if ragged else UNIFORM) and state["classnames"] is None
    assert state["shots"].tolist() == (RAGGED[:6] if ragged else [UNIFORM] * 6) and state["features"].shape == (int(state["shots"].sum()), SPEC.embed_dim)
    assert state["exemplar_paths"] is None and state["n_ctx"] == N_CTX and state["embed_dim"] == SPEC.embed_dim
    m2 = _model([8, 7, 6], str(d / "loaded"), ragged=ragged)
    m2.engine.calls.clear()
    m2.load_bank(str(d / "gen" / bank.BANK_FILE))
    assert [c for c, _ in m2.engine.calls] == ["embed_tokens"]              # the vocabulary's embedding, nothing else
    _same_state(m, m2, "round trip")
    _vocabulary_is_consistent(m2, 6)
    m2.engine.calls.clear()
    assert torch.equal(m2(QUERY), m(QUERY))
    assert {c for c, _ in m2.engine.calls} == {"encode_image", "fused_logits"}
    m2.save_classifiers()
    _same_files(str(d / "gen"), str(d / "loaded"), "round trip")
    _counters_are_a_function_of_the_state(m2)


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_aligned_edits_equal_the_from_scratch_job(generated, ragged, tmp_path):
    """Points 2, 3 and 4: add two classes, remove the first and the last, replace one -- one class per loader batch and no longer prompt, so
    every edit is aligned: after each step the model equals the from-scratch job on the same final state, tensors and files, and every
    class that was not named kept its rows bit for bit."""
    _, d = generated[ragged]
    m = _model([0], str(tmp_path / "edited"), ragged=ragged)
    m.load_bank(str(d / "gen" / bank.BANK_FILE))
    m.engine.calls.clear()

    def check(step, classes, untouched_before, untouched_now, old_rows):
        _vocabulary_is_consistent(m, len(classes))
        for a, b in zip(old_rows, _rows_of(m, untouched_now)):
            assert torch.equal(a, b), f"{step}: an old class's rows changed"
        _counters_are_a_function_of_the_state(m)
        ref = _scratch(classes, ragged, str(tmp_path / f"scratch_{step}"))
        _same_state(m, ref, step)
        m.save_classifiers()
        _same_files(str(tmp_path / "edited"), str(tmp_path / f"scratch_{step}"), step)
        assert torch.equal(m(QUERY), ref(QUERY)), step

    old = _rows_of(m, list(range(6)))
    m.add_classes(_rows([6, 7]), OneClassPerBatch([6, 7], ragged))
    n_new = sum(RAGGED[6:8]) if ragged else 2 * UNIFORM
    assert [c for c, _ in m.engine.calls].count("encode_image") == 2           # the two new classes' batches, nothing of an old class
    assert m.eval_feat4cls.shape[0] == (sum(RAGGED[:6]) if ragged else 6 * UNIFORM) + n_new
    check("add", list(range(8)), list(range(6)), list(range(6)), old)

    old = _rows_of(m, list(range(1, 7)))
    m.engine.calls.clear()
    m.remove_classes([7, 0])
    assert {c for c, _ in m.engine.calls} == {"xval_counts", "fusion_weights"}      # nothing is encoded or generated
    check("remove", list(range(1, 7)), list(range(1, 7)), list(range(6)), old)

    keep = [0, 1, 3, 4, 5]                                                      # label 2 is class 3 of the pool
    old = _rows_of(m, keep)
    m.replace_classes([2], OneClassPerBatch([(3, 1)], ragged))
    check("replace", [1, 2, (3, 1), 4, 5, 6], keep, keep, old)


def test_unaligned_add_meets_the_bar(generated, tmp_path):
    """Point 5: a class whose name tokenises longer than every old one raises max_eos, hence the truncated tower lengths of the NEW rows;
    the old rows stay as they are.  Every classifier row and visual token is within 1 - cos <= 1e-3 of the from-scratch job's, and the
    counters are what the state gives (the fusion weights are not compared: a near-tie may flip a counter)."""
    _, d = generated[True]
    m = _model([0])
    m.load_bank(str(d / "gen" / bank.BANK_FILE))
    old, eos = _rows_of(m, list(range(6))), m.prompt_learner.max_eos
    m.add_classes(_rows([8]), OneClassPerBatch([8], True))
    assert m.prompt_learner.max_eos == eos + 2
    for a, b in zip(old, _rows_of(m, list(range(6)))):
        assert torch.equal(a, b)
    _counters_are_a_function_of_the_state(m)
    ref = _scratch([0, 1, 2, 3, 4, 5, 8], True)
    for name in ("mm_classifier", "visual_classifer", "zero_shot_classifier", "visual_tokens"):
        assert_cosine(getattr(m, name).float().flatten(0, -2).numpy(), getattr(ref, name).float().flatten(0, -2).numpy(), COS_TOL, name)


def test_bank_under_another_tau(generated):
    """A bank loaded under another EVAL_TAU: the fusion weights are recomputed from the stored counters and equal a generation under that tau."""
    m, d = generated[True]
    ref = _scratch(range(6), True, tau=3.0)
    assert not torch.equal(ref.fusion_weight, m.fusion_weight)
    m2 = _model([0], tau=3.0)
    m2.load_bank(str(d / "gen" / bank.BANK_FILE))
    _same_state(m2, ref, "tau 3")
    assert m2.bank_state()["tau"] == 3.0


def test_reserve_crossing_refinalizes_once(generated):
    """Reserve (8, 8, 6) and 6 -> 8 classes: the engine is re-finalised exactly once, at 8, before the edit's first launch; a removal and an
    add that fits do not finalise again."""
    _, d = generated[False]
    m = _model([0], reserve=(8, 8, 6), ragged=False)
    m.load_bank(str(d / "gen" / bank.BANK_FILE))
    e = m.engine
    e.calls.clear()
    m.add_classes(_rows([6, 7]), OneClassPerBatch([6, 7], False))
    assert [a for c, a in e.calls if c == "finalize"] == [(8, 8, 8)] and e.calls[0][0] == "finalize" and e._reserve == (8, 8, 8)
    e.calls.clear()
    m.remove_classes([0])
    m.add_classes(_rows([8]), OneClassPerBatch([8], False))
    assert not [c for c, _ in e.calls if c == "finalize"]
    m3 = _model([0], reserve=(8, 8, 4))                                     # a bank beyond the reserve: load_bank raises it
    m3.engine.calls.clear()
    m3.load_bank(str(d / "gen" / bank.BANK_FILE))
    assert m3.engine.calls[0] == ("finalize", (8, 8, 6)) and [c for c, _ in m3.engine.calls].count("finalize") == 1


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_come_before_any_launch(generated, tmp_path):
    _, d = generated[True]
    path = str(d / "gen" / bank.BANK_FILE)
    m = _model([0])
    m.load_bank(path)
    e = m.engine
    e.calls.clear()
    state = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in m.bank_state().items()}
    one = OneClassPerBatch([6], True)

    def refused(match, call, *a, **kw):
        with pytest.raises(ValueError, match=match) as err:
            call(*a, **kw)
        assert "\n" not in str(err.value) and e.calls == [], match

    refused("in the vocabulary already \\(label 3\\)", m.add_classes, _rows([6, 3]), OneClassPerBatch([6, 3], True))
    refused("given twice", m.add_classes, _rows([6, 6]), OneClassPerBatch([6, 6], True))
    refused("unknown class name 'tench'", m.replace_classes, ["tench"], one)
    refused("unknown class name 'tench'", m.remove_classes, ["tench"])
    refused("label 6 outside \\[0, 6\\)", m.replace_classes, [6], one)
    refused("label -1 outside", m.remove_classes, [2, -1])
    refused("named twice", m.remove_classes, [2, 2])
    refused("no tokenizer", m.add_classes, ["tench"], one)
    refused("every class", m.remove_classes, list(range(6)))
    too_many = OneClassPerBatch([6], True)
    too_many.shots = torch.tensor([CAP + 1], dtype=torch.int32)
    refused(f"more than DATASET.NUM_SHOTS = {CAP}", m.add_classes, _rows([6]), too_many)
    refused("describes 1 classes, 2 are named", m.add_classes, _rows([6, 7]), one)
    m.aug_times = 2
    refused("K_TRANSFORMS", m.add_classes, _rows([6]), one)
    refused("K_TRANSFORMS", m.replace_classes, [0], one)
    refused("K_TRANSFORMS", m.remove_classes, [0])
    m.aug_times = 1
    m._dist = SimpleNamespace(get_world_size=lambda: 2, get_rank=lambda: 0)
    for call, a in ((m.add_classes, (_rows([6]), one)), (m.replace_classes, ([0], one)), (m.remove_classes, ([0],)), (m.save_bank, (str(tmp_path / "b.pt"),)),
                    (m.load_bank, (path,))):
        refused("more than one rank", call, *a)
    m._dist = None
    for k, v in m.bank_state().items():                                     # nothing of it changed the model
        assert torch.equal(v, state[k]) if isinstance(v, torch.Tensor) else v == state[k], k
    # a model without classifiers, and one that only has load_classifiers state
    fresh = _model(list(range(6)))
    fresh.engine.calls.clear()
    e = fresh.engine
    for call, a in ((fresh.add_classes, (_rows([6]), one)), (fresh.replace_classes, ([0], one)), (fresh.remove_classes, ([0],)),
                    (fresh.save_bank, (str(tmp_path / "b.pt"),))):
        refused("no classifiers yet", call, *a)
    fresh.load_classifiers(str(d / "gen" / "mm_classifiers.pt"))
    for call, a in ((fresh.add_classes, (_rows([6]), one)), (fresh.remove_classes, ([0],)), (fresh.save_bank, (str(tmp_path / "b.pt"),))):
        refused("no exemplar features", call, *a)
    assert not (tmp_path / "b.pt").exists()


def test_a_failed_edit_leaves_the_model_as_it_was(generated):
    """A loader that brings no rows for a named class fails AFTER the buffers have grown: the model is restored."""
    _, d = generated[False]
    m = _model([0], ragged=False)
    m.load_bank(str(d / "gen" / bank.BANK_FILE))
    state = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in m.bank_state().items()}
    short = OneClassPerBatch([6, 7], False)
    short.classes = short.classes[:1]
    with pytest.raises(ValueError, match="no exemplar for class 1"):
        m.add_classes(_rows([6, 7]), short)
    _vocabulary_is_consistent(m, 6)
    for k, v in m.bank_state().items():
        assert torch.equal(v, state[k]) if isinstance(v, torch.Tensor) else v == state[k], k


def test_loader_refuses_what_is_not_this_models_bank(generated, tmp_path):
    """The fingerprint tells another prompt-learner state and another CLIP state apart; a file that is no bank, a newer format, another
    n_ctx and another width are refused with the file and the field."""
    m, d = generated[False]
    path = str(d / "gen" / bank.BANK_FILE)
    assert m.model_fingerprint() == _model([0]).model_fingerprint() == bank.read(path)["fingerprint"]
    for kw in ({"pl_seed": SEED + 1}, {"clip_seed": SEED + 1}):
        other = _model(list(range(6)), **kw)
        assert other.model_fingerprint() != m.model_fingerprint()
        other.engine.calls.clear()
        with pytest.raises(ValueError, match="reference_bank.pt.*fingerprint"):
            other.load_bank(path)
        assert other.engine.calls == [] and other.mm_classifier is None
    # every single tensor of either state dict moves the fingerprint
    pl, clip = m.prompt_learner.state_dict(), m.prompt_learner.clip_model.state_dict()
    base = bank.fingerprint(SPEC, N_CTX, pl, clip)
    assert base == m.model_fingerprint() and bank.fingerprint(SPEC, N_CTX + 1, pl, clip) != base
    for sd, keys in ((pl, sorted(pl)), (clip, bank.FINGERPRINT_CLIP_KEYS)):
        for k in keys:
            moved = dict(sd)
            moved[k] = sd[k].clone()
            moved[k].view(-1)[0] += 0.5
            assert bank.fingerprint(SPEC, N_CTX, *((moved, clip) if sd is pl else (pl, moved))) != base, k
    target = _model([0])
    with pytest.raises(ValueError, match="mm_classifiers.pt.*format.*not a reference bank"):
        target.load_bank(str(d / "gen" / "mm_classifiers.pt"))
    good = torch.load(path)
    wider = {k: torch.cat([good[k], good[k]], -1) for k in ("features", "mm_classifier", "vision_classifier", "text_classifier", "visual_tokens")}
    for change, match in (({"format": bank.BANK_FORMAT + 1}, "format is 2"),
                          ({"n_ctx": N_CTX + 1, "visual_tokens": torch.cat([good["visual_tokens"], good["visual_tokens"][:, :1]], 1)}, "n_ctx is 3"),
                          (dict(wider, embed_dim=SPEC.embed_dim * 2), "embed_dim is 256"), ({"shots": good["shots"][:-1]}, "shots"),
                          ({"mm_classifier": good["mm_classifier"][:-1]}, "mm_classifier is \\[5, 128\\]")):
        torch.save(dict(good, **change), tmp_path / "bad.pt")
        with pytest.raises(ValueError, match="bad.pt.*" + match):
            target.load_bank(str(tmp_path / "bad.pt"))
    assert target.mm_classifier is None


# ---- class names ---------------------------------------------------------------------------------------------------------------------

def test_edits_by_class_name(tmp_path):
    """A model built from class names keeps the list through bank and edits; names address replace and remove; a known name is refused."""
    names = ["tench", "great white shark", "stop sign", "yin yang"]
    tk = WordTokenizer()
    loader = OneClassPerBatch([0, 1, 2, 3], False)
    m = _model(names, str(tmp_path / "gen"), tokenizer=tk, ragged=False)
    m.forward_prompt(loader)
    m.save_bank(str(tmp_path / "bank.pt"), exemplar_paths=[f"c{c}/{i}.png" for c in range(4) for i in range(UNIFORM)])
    with pytest.raises(ValueError, match="4 exemplar paths for 12"):
        m.save_bank(str(tmp_path / "bank2.pt"), exemplar_paths=["a", "b", "c", "d"])
    m2 = _model(["sea horse"], tokenizer=tk, ragged=False)
    m2.load_bank(str(tmp_path / "bank.pt"))
    assert m2.classnames == names and m2.bank_state()["exemplar_paths"][:5] == ["c0/0.png", "c0/1.png", "c0/2.png", "c1/0.png", "c1/1.png"]
    m2.engine.calls.clear()
    with pytest.raises(ValueError, match="'stop sign' is in the vocabulary already \\(label 2\\)"):
        m2.add_classes(["sea horse", "stop sign"], OneClassPerBatch([6, 7], False))
    with pytest.raises(ValueError, match="in the vocabulary already"):      # another spelling of the same prompt
        m2.add_classes(["stop_sign"], OneClassPerBatch([6], False))
    with pytest.raises(ValueError, match="pass names, not token rows"):
        m2.add_classes(_rows([6]), OneClassPerBatch([6], False))
    assert m2.engine.calls == []
    m2.add_classes(["sea horse", "lion"], OneClassPerBatch([6, 7], False), exemplar_paths=[["s/0"] * UNIFORM, ["l/0"] * UNIFORM])
    m2.remove_classes(["tench", "stop sign"])
    m2.replace_classes(["lion"], OneClassPerBatch([(7, 1)], False), exemplar_paths=[["l/1"] * UNIFORM])
    final = ["great white shark", "yin yang", "sea horse", "lion"]
    assert m2.classnames == final and m2.bank_state()["exemplar_paths"][-UNIFORM:] == ["l/1"] * UNIFORM
    _vocabulary_is_consistent(m2, 4)
    ref = _model(final, tokenizer=tk, ragged=False)
    ref.forward_prompt(OneClassPerBatch([1, 3, 6, (7, 1)], False))
    for k in bank.TENSORS:                                                  # (the longest name is in both vocabularies throughout: aligned)
        assert torch.equal(m2.bank_state()[k], ref.bank_state()[k]), k
    m2.save_bank(str(tmp_path / "bank3.pt"))
    assert bank.read(str(tmp_path / "bank3.pt"))["classnames"] == final


# ---- the runner ----------------------------------------------------------------------------------------------------------------------

def test_runner_flag_refusals(tmp_path, monkeypatch):
    """One-line SystemExits before any image is listed (no data set, no weights file exist here)."""
    from ovmr_amd import cli
    base = ["--clip-weights", "none.pt", "--eval-only", "--root", str(tmp_path / "no_data")]
    mm, zs = ["--trainer", "MM_CLS_OP"], ["--trainer", "ZeroshotCLIP", "DATASET.NAME", "Caltech101"]
    (tmp_path / "bank.pt").write_bytes(b"")
    for argv, match in ((mm + ["--add-classes", "d"], "give --bank FILE"), (mm + ["--replace-classes", "d"], "give --bank FILE"),
                        (mm + ["--remove-classes", "a", "b"], "give --bank FILE"),
                        (["--bank", str(tmp_path / "bank.pt")] + zs, "ZeroshotCLIP has no generated vocabulary"),
                        (["--save-bank"] + zs, "ZeroshotCLIP has no generated vocabulary"),
                        (mm + ["--bank", str(tmp_path / "missing.pt")], "no such file"),
                        (mm + ["--bank", str(tmp_path / "bank.pt"), "--save-bank"], "belongs to a generation job"),
                        (mm + ["--bank", str(tmp_path / "bank.pt"), "--predict", str(tmp_path), "--classifiers", "x"], "not together with --classifiers")):
        with pytest.raises(SystemExit) as err:
            cli.main(base + argv)
        assert match in str(err.value) and "\n" not in str(err.value), argv
    monkeypatch.setenv("WORLD_SIZE", "2")
    for argv in (mm + ["--save-bank"], mm + ["--bank", str(tmp_path / "bank.pt")]):
        with pytest.raises(SystemExit, match="one process"):
            cli.main(base + argv)


def test_runner_plans_edits_from_folders(tmp_path):
    """--add-classes / --replace-classes folders: sorted folder order, names from classnames.txt, the draw of build_splits; the plan's
    refusals name the class."""
    from test_ragged_cpu import _folder
    from ovmr_amd import cli
    add = tmp_path / "add"
    add.mkdir()
    items = _folder(add, [3, 6])
    (add / "classnames.txt").write_text("c1 sea horse\n")
    names, laid = cli.list_edit_classes(str(add), 4, 1)
    assert names == ["c0", "sea horse"] and [l for _, l in laid] == [0] * 4 + [1] * 4 and len(set(laid)) == 3 + 4
    assert laid == cli.layout_exemplars(cli.fewshot_items(items, 4, 1), 4, 1)
    names, laid = cli.list_edit_classes(str(add), 4, 1, ragged=True)
    assert [l for _, l in laid] == [0] * 3 + [1] * 4 and laid == cli.fewshot_items(items, 4, 1)
    args = SimpleNamespace(remove_classes=["b"], replace_classes="", add_classes=str(add))
    remove, replace, added, final = cli.plan_vocabulary_edits(args, ["a", "b", "c"], 4, 1, False)
    assert remove == ["b"] and replace is None and added[0] == ["c0", "sea horse"] and final == ["a", "c", "c0", "sea horse"]
    for kw, have, match in (({"remove_classes": ["x"]}, ["a"], "no class 'x'"), ({"remove_classes": ["a"]}, ["a"], "every class"),
                            ({"add_classes": str(add)}, ["a", "sea horse"], "'sea horse' is in the vocabulary already"),
                            ({"replace_classes": str(add)}, ["a", "c0"], "no class 'sea horse'"),
                            ({"add_classes": str(tmp_path / "nope")}, ["a"], "no such directory")):
        with pytest.raises(SystemExit, match=match):
            cli.plan_vocabulary_edits(SimpleNamespace(**{"remove_classes": None, "replace_classes": "", "add_classes": "", **kw}), have, 4, 1, False)
    (add / "empty").mkdir()
    with pytest.raises(SystemExit, match="'empty' holds no image"):
        cli.list_edit_classes(str(add), 4, 1)
    assert bank.first_difference(["a", "b"], ["a", "b"]) is None and "class 1 is 'b'" in bank.first_difference(["a", "b"], ["a", "c"])
    assert "2 classes" in bank.first_difference(["a", "b"], ["a"])
