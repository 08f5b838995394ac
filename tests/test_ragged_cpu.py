"""Ragged exemplar sets without a GPU: the runner's layout and loaders (whole classes per batch, the "shots" key, `.shots`), and the
Python layer of ovmr_amd.modules on the CPU stand-in engine of tests/test_distributed_cpu.py -- one process and gloo worlds of 2 and 3
ranks must end with the same bits, a batch without "shots" must take the uniform path unchanged."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import REPO
from ovmr_amd import synth
from test_distributed_cpu import N_CTX, SEED, FakeCLIPModel, OracleEngine, _free_port

SHOTS = [3, 1, 4, 2, 4, 1, 2]                 # 7 classes, 17 rows: worlds of 2 and 3 ranks own 4 + 3 and 3 + 2 + 2 classes
CAP = 4                                       # DATASET.NUM_SHOTS of the ragged jobs: the most a class may bring


# ---- the runner's layout -------------------------------------------------------------------------------------------------------

def _items(per_class):
    return [(f"c{c}/im{i}.jpg", c) for c, n in per_class for i in range(n)]


def test_layout_exemplars_ragged():
    from ovmr_amd import cli
    few = _items([(2, 3), (0, 1), (5, 4)])
    few = few[:1] + few[3:4] + few[1:3] + few[4:]                 # class 0's row between class 2's rows
    out = cli.layout_exemplars_ragged(few, 4)
    assert [l for _, l in out] == [2, 2, 2, 0, 5, 5, 5, 5]        # classes in order of first appearance, rows consecutive
    assert [p for p, l in out if l == 2] == ["c2/im0.jpg", "c2/im1.jpg", "c2/im2.jpg"]      # ... in the order given
    assert len(set(out)) == len(out) == len(few)                  # nothing filled, nothing dropped
    filled = cli.layout_exemplars(few, 4, seed=1)                 # the uniform layout of the same rows: 4 per class, duplicates
    assert len(filled) == 12 and len(set(filled)) == len(few)
    with pytest.raises(ValueError, match="more than DATASET.NUM_SHOTS = 3"):
        cli.layout_exemplars_ragged(few, 3)
    with pytest.raises(ValueError, match="twice"):
        cli.layout_exemplars_ragged(few + few[:1], 4)
    # the draw itself is fewshot_items': a short class keeps what it has, a long one is sampled down to the cap
    pool = _items([(0, 2), (1, 9)])
    drawn = cli.layout_exemplars_ragged(cli.fewshot_items(pool, 4, seed=1), 4)
    assert [l for _, l in drawn] == [0, 0, 1, 1, 1, 1] and drawn == cli.fewshot_items(pool, 4, seed=1)


def test_ragged_batches_and_vocabulary_shots():
    from ovmr_amd.shard import ragged_batches, vocabulary_shots
    items = _items([(0, 3), (1, 1), (2, 4), (3, 2), (4, 4), (5, 1), (6, 2)])
    spans = ragged_batches(items, 5)
    assert spans == [(0, 4, [3, 1]), (4, 8, [4]), (8, 10, [2]), (10, 15, [4, 1]), (15, 17, [2])]
    assert all(b - a <= 5 and sum(s) == b - a for a, b, s in spans)
    assert ragged_batches(items, 17) == [(0, 17, SHOTS)] and ragged_batches([], 4) == []
    with pytest.raises(ValueError, match="class 2 has 4 exemplar rows, more than one batch"):
        ragged_batches(items, 3)
    with pytest.raises(ValueError, match="consecutively"):
        ragged_batches(items + items[:1], 5)
    assert vocabulary_shots(items, 9).tolist() == SHOTS + [0, 0] and vocabulary_shots(items, 9).dtype == torch.int32


def _folder(tmp_path, per_class):
    from PIL import Image
    rng = np.random.default_rng(0)
    items = []
    for c, n in enumerate(per_class):
        d = tmp_path / f"c{c}"
        d.mkdir()
        for i in range(n):
            Image.fromarray(rng.integers(0, 255, (20, 24, 3), dtype=np.uint8)).save(d / f"im{i}.png")
            items.append((str(d / f"im{i}.png"), c))
    return items


def test_loaders_emit_whole_classes(tmp_path):
    from ovmr_amd import cli
    from ovmr_amd.loader import PipelinedFolderLoader
    items = _folder(tmp_path, SHOTS)
    fl = cli.FolderLoader(items, 5, 16, ragged=True, num_classes=7)
    assert fl.shots.tolist() == SHOTS and fl.shots.dtype == torch.int32 and len(fl) == 5
    batches = list(fl)
    assert [b["shots"].tolist() for b in batches] == [[3, 1], [4], [2], [4, 1], [2]]
    for b in batches:
        assert b["shots"].dtype == torch.int64 and not b["shots"].is_cuda
        assert b["img"].shape[0] == b["label"].shape[0] == int(b["shots"].sum()) <= 5
        assert b["label"].tolist() == sorted(b["label"].tolist())
    assert torch.cat([b["label"] for b in batches]).tolist() == [l for _, l in items]
    # rank 1 of 2 owns classes 4..6 and still knows the whole vocabulary's shots
    r1 = cli.FolderLoader(items, 5, 16, 1, 2, 7, ragged=True)
    assert r1.presharded and r1.shots.tolist() == SHOTS and [s for _, _, s in r1.spans] == [[4, 1], [2]]
    for make in (lambda **kw: cli.FolderLoader(items, 3, 16, **kw), lambda **kw: PipelinedFolderLoader(items, 3, 16, **kw)):
        with pytest.raises(ValueError, match="more than one batch"):       # a class larger than the batch: refused up front
            make(ragged=True, num_classes=7)
        assert "shots" not in make().__dict__ or make().shots is None      # uniform loaders publish no per-class shots
    pl = PipelinedFolderLoader(items, 5, 16, 1, 2, 7, ragged=True)         # (nothing is decoded before iteration: no GPU needed here)
    assert pl.shots.tolist() == SHOTS and pl.spans == r1.spans and len(pl) == 2
    uniform = PipelinedFolderLoader(items, 5, 16)
    assert [(a, b) for a, b, _ in uniform.spans] == [(0, 5), (5, 10), (10, 15), (15, 17)] and len(uniform) == 4
    assert "shots" not in next(iter(cli.FolderLoader(items, 5, 16)))


def test_build_splits_ragged(tmp_path):
    """--ragged-shots: min(available, NUM_SHOTS) images per class, unfilled; an --exemplar-list with fewer rows per class is taken as
    it is, more than NUM_SHOTS is still refused; a class with no exemplar exits with its name."""
    from types import SimpleNamespace
    from ovmr_amd import cli
    root = tmp_path / "data"
    (root / "train").mkdir(parents=True)
    items = _folder(root / "train", [2, 6, 1])
    cfg = SimpleNamespace(DATASET=SimpleNamespace(NUM_SHOTS=4, SUBSAMPLE_CLASSES="all", ROOT=str(root)), SEED=1)
    names, ex, _ = cli.build_splits(cfg, "train", None, "", ragged=True)
    assert names == ["c0", "c1", "c2"] and [l for _, l in ex] == [0, 0, 1, 1, 1, 1, 2] and len(set(ex)) == 7
    assert ex == cli.fewshot_items(items, 4, 1)                          # drawn as exemplar_items draws, then nothing added
    assert len(cli.build_splits(cfg, "train", None, "")[1]) == 12         # the uniform layout fills to 4 per class
    lst = tmp_path / "list.txt"
    lst.write_text("".join(f"{p} {l}\n" for p, l in items if l != 1 or p.endswith(("im0.png", "im4.png"))))
    assert [l for _, l in cli.build_splits(cfg, "train", None, str(lst), ragged=True)[1]] == [0, 0, 1, 1, 2]
    lst.write_text("".join(f"{p} {l}\n" for p, l in items))
    with pytest.raises(SystemExit, match="more than DATASET.NUM_SHOTS = 4"):
        cli.build_splits(cfg, "train", None, str(lst), ragged=True)
    lst.write_text("".join(f"{p} {l}\n" for p, l in items if l == 0))
    with pytest.raises(SystemExit, match="no exemplar image for class 'c1'"):
        cli.build_splits(cfg, "train", None, str(lst), ragged=True)
    assert cli.parse(["--clip-weights", "x", "--ragged-shots"]).ragged_shots is True


# ---- the Python layer on the CPU stand-in ----------------------------------------------------------------------------------------

class RaggedOracleEngine(OracleEngine):
    """The stand-in with generate_tokens_ragged.  torch's CPU GEMMs are not batch-invariant, the HIP kernels' rows are: every call
    here runs image by image, prompt by prompt and class by class (a group of one shot count at a time), so that a class's bits do not
    depend on which batch or rank it came through -- which is what the comparison between worlds is about."""
    ragged_calls = 0

    def encode_image(self, img, normalize=True, out=None):
        return torch.cat([OracleEngine.encode_image(self, img[i:i + 1], normalize) for i in range(img.shape[0])]) if img.shape[0] else \
            torch.zeros((0, self.spec.embed_dim), dtype=torch.float16)

    def generate_tokens(self, feats):
        return torch.cat([OracleEngine.generate_tokens(self, feats[c:c + 1]) for c in range(feats.shape[0])])

    def generate_tokens_ragged(self, feats, shots):
        type(self).ragged_calls += 1
        assert feats.dim() == 2 and sum(shots) == feats.shape[0]
        return torch.cat([OracleEngine.generate_tokens(self, rows.unsqueeze(0)) for rows in torch.split(feats, list(shots))])

    def encode_text_groups(self, groups):
        outs = []
        for g in groups:
            n = (g["ids"] if g.get("ids") is not None else g["prompts"]).shape[0]
            one = [OracleEngine.encode_text_groups(self, [{k: (v[i:i + 1] if isinstance(v, torch.Tensor) else v) for k, v in g.items()}])[0]
                   for i in range(n)]
            outs.append(torch.cat(one))
        return outs


class RaggedClipModel(FakeCLIPModel):
    def engine(self, n_ctx):
        if n_ctx not in self._e:
            self._e[n_ctx] = RaggedOracleEngine(self.spec, n_ctx)
        return self._e[n_ctx]


class ListLoader:
    """A ragged (or, shots=None, uniform) eval-set loader over resident images: the protocol of cli.FolderLoader."""

    def __init__(self, img, labels, batch, rank=0, world=1, num_classes=0, ragged=True, presharded=None):
        from ovmr_amd.shard import ragged_batches, shard_range, vocabulary_shots
        items = [(i, int(l)) for i, l in enumerate(labels)]
        self.presharded = world > 1 if presharded is None else presharded
        if ragged:
            self.shots = vocabulary_shots(items, num_classes)
        if self.presharded:
            lo, hi = shard_range(num_classes, rank, world)
            items = [it for it in items if lo <= it[1] < hi]
        self.items, self.img = items, img
        self.spans = ragged_batches(items, batch) if ragged else [(s, min(s + batch, len(items)), None) for s in range(0, len(items), batch)]

    def __iter__(self):
        for a, b, shots in self.spans:
            rows = [i for i, _ in self.items[a:b]]
            batch = {"img": self.img[rows], "label": torch.tensor([l for _, l in self.items[a:b]])}
            if shots is not None:
                batch["shots"] = torch.tensor(shots, dtype=torch.long)
            yield batch


def _job(shots, outdir="", num_shots=CAP):
    from ovmr_amd import modules
    spec, C = synth.SPECS["tiny"], len(shots)
    cfg = modules.make_cfg(n_ctx=N_CTX, num_shots=num_shots, output_dir=outdir, test_batch_size=6)
    pl = {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, N_CTX, SEED, True).items()}
    tok = torch.from_numpy(synth.class_token_ids(C, seed=4321))
    model = modules.CustomCLIP(cfg, tok, RaggedClipModel(spec), prompt_learner_state=pl, reserve=(8, 8, 8))
    labels = np.repeat(np.arange(C), shots)
    img = torch.from_numpy(synth.images(len(labels), spec.image_resolution, 1234, labels, 0.6))
    return model, img, labels


def _state(model):
    return {"mm": model.mm_classifier, "v": model.visual_classifer, "t": model.zero_shot_classifier, "w": model.fusion_weight,
            "counts": model.xval_counts, "tokens": model.visual_tokens}


def _run(rank, world, port, outdir, result, presharded=True):
    sys.path.insert(0, REPO)
    torch.set_num_threads(2)
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
    model, img, labels = _job(SHOTS, outdir if rank == 0 else "")
    loader = ListLoader(img, labels, 6, rank, world, len(SHOTS), presharded=presharded and world > 1)
    if not presharded:
        try:
            model.forward_prompt(loader)
            raised = ""
        except RuntimeError as e:
            raised = str(e)
        torch.save(raised, f"{result}.{rank}")
    else:
        model.forward_prompt(loader)
        w_gen = model.fusion_weight.clone()
        w_coop = model.get_fusion_weight(loader, model.mm_classifier.float(), model.visual_classifer, model.zero_shot_classifier)
        assert torch.equal(w_coop, w_gen)
        if rank == 0:
            torch.save(_state(model), result)
    if world > 1:
        if presharded:
            dist.barrier()
        dist.destroy_process_group()


@pytest.fixture(scope="module", autouse=True)
def _two_threads():
    """The thread count of the spawned ranks, for everything this module computes in-process: torch's CPU sums depend on it."""
    threads = torch.get_num_threads()
    torch.set_num_threads(2)
    yield
    torch.set_num_threads(threads)


@pytest.fixture(scope="module")
def single():
    """The ragged job in one process: computed once, shared."""
    with tempfile.TemporaryDirectory() as d:
        model, img, labels = _job(SHOTS, os.path.join(d, "o1"))
        model.forward_prompt(ListLoader(img, labels, 6, num_classes=len(SHOTS)))
        saved = torch.load(os.path.join(d, "o1", "mm_classifiers.pt"))
        tokens_file = torch.load(os.path.join(d, "o1", "visual_tokens.pt"))
    return model, saved, tokens_file


def test_ragged_job_one_process(single):
    model, saved, tokens_file = single
    C, R, D = len(SHOTS), sum(SHOTS), synth.SPECS["tiny"].embed_dim
    assert model.eval_feat4cls.shape == (R, D) and model.eval_row_labels.tolist() == np.repeat(np.arange(C), SHOTS).tolist()
    counts = model.xval_counts
    assert counts[:, 1].sum(-1).tolist() == [R, R, R]                       # every row voted once per classifier: no duplicate rows
    assert bool((counts[:, 0] <= torch.tensor(SHOTS)).all())                # tp[c] <= shots[c]
    from oracle import ovmr_oracle as O
    f1 = torch.stack([O.f1_from_counts(counts[m, 0], counts[m, 1], torch.tensor(SHOTS)) for m in range(3)], -1)
    assert torch.allclose(model.fusion_weight, (10.0 * f1).softmax(-1), atol=1e-6)
    # per class, the tokens are the stand-in's uniform call on the class's own rows: PromptLearner.forward at num_ins = shots[c]
    e = model.engine
    for c, rows in enumerate(torch.split(model.eval_feat4cls, SHOTS)):
        assert torch.equal(model.visual_tokens[c], e.generate_tokens(rows.unsqueeze(0))[0].half()), c
    # the output files keep their keys, dtypes and shapes
    assert sorted(saved) == ["fusion_weight", "mm_classifier", "text_classifier", "vision_classifier"]
    assert all(saved[k].dtype == torch.float32 for k in saved) and saved["mm_classifier"].shape == (C, D) and saved["fusion_weight"].shape == (C, 3)
    assert tokens_file["visual_tokens"].shape == (C, N_CTX, D) and tokens_file["visual_tokens"].dtype == torch.float16


@pytest.mark.timeout(900)
@pytest.mark.parametrize("world", [2, 3])
def test_ragged_job_matches_across_worlds(single, world):
    a = _state(single[0])
    with tempfile.TemporaryDirectory() as d:
        r2 = os.path.join(d, "dist.pt")
        mp.spawn(_run, args=(world, _free_port(), os.path.join(d, "o2"), r2), nprocs=world, join=True)
        b = torch.load(r2)
        for k in a:
            assert torch.equal(a[k], b[k]), k
        assert sorted(torch.load(os.path.join(d, "o2", "mm_classifiers.pt"))) == ["fusion_weight", "mm_classifier", "text_classifier", "vision_classifier"]


@pytest.mark.timeout(600)
def test_ragged_needs_a_presharded_loader_with_several_ranks():
    """A round-robin loader in ragged mode: every rank raises, before the first collective (no rank is left waiting in one)."""
    with tempfile.TemporaryDirectory() as d:
        r = os.path.join(d, "raised")
        mp.spawn(_run, args=(2, _free_port(), "", r, False), nprocs=2, join=True)
        for rank in range(2):
            assert "presharded" in torch.load(f"{r}.{rank}"), rank


def test_ragged_refuses_k_transforms_and_mixed_loaders():
    model, img, labels = _job(SHOTS)
    loader = list(ListLoader(img, labels, 6, num_classes=len(SHOTS)))
    with pytest.raises(NotImplementedError, match="K_TRANSFORMS"):
        model.forward_prompt([dict(loader[0], img=[loader[0]["img"], loader[0]["img"]])])
    with pytest.raises(RuntimeError, match="one mode per loader"):
        model.forward_prompt([loader[0], {k: v for k, v in loader[1].items() if k != "shots"}])


def test_batches_without_shots_take_the_uniform_path():
    """Nothing existing moved: a loader whose batches carry no "shots" runs the uniform code (the [C, S, D] exemplar buffer, n_label = S,
    no ragged call), and its result is, bit for bit, the ragged job's on the same all-equal counts."""
    S, C = 4, 5
    model, img, labels = _job([S] * C, num_shots=S)
    RaggedOracleEngine.ragged_calls = 0
    model.forward_prompt(ListLoader(img, labels, 8, num_classes=C, ragged=False))
    assert RaggedOracleEngine.ragged_calls == 0 and model.eval_feat4cls.shape[:2] == (C, S) and model.eval_row_labels is None
    uniform = {k: v.clone() for k, v in _state(model).items()}
    model.forward_prompt(ListLoader(img, labels, 8, num_classes=C))
    assert RaggedOracleEngine.ragged_calls == 3 and model.eval_feat4cls.shape[0] == C * S
    for k, v in _state(model).items():
        assert torch.equal(v, uniform[k]), k
