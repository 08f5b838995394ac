"""Nearest exemplars through the model and the runner (tiny / small synthetic models, the real library): CustomCLIP.nearest_exemplars over
the uniform and the packed exemplar store, the per-class form against the whole-bank call on that class's rows, predict_explained against
predict_topk, the refusals, and `--predict ... --nearest N` (neighbours.csv next to an unchanged predictions.csv).  The kernel itself is
held to exact values by test_hip_nearest.py.  Run with -m gpu on an MI355X."""
import csv

import numpy as np
import pytest
import torch

import nearest_cases as N
from ovmr_amd import bank, synth
from test_bank_cpu import _rows
from test_hip_bank import OLD, QUERIES, S, SEED, SPEC, _class_folders, _clip, _model, _pl_state, _scratch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clip():
    return _clip()


def _plant_duplicate(m, lo, hi):
    """Bank row hi becomes a copy of row lo (rows in label order: the generation's loaders go class after class)."""
    store = m.eval_feat4cls
    flat = store.view(-1, store.shape[-1])
    flat[hi] = flat[lo]
    m.__dict__.pop("_nearest_bank", None)


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_own_feature_first_and_per_class_form(ragged, clip):
    from ovmr_amd import runtime
    m = _scratch(range(6), ragged, "", clip)
    R = int(m._exemplar_bank()[1][-1])
    lo, hi = 3, R - 2
    _plant_duplicate(m, lo, hi)
    bnk, starts = m._exemplar_bank()
    starts = starts.cpu()
    assert bnk.shape == (R, SPEC.embed_dim) and starts.tolist() == ([0, 2, 4, 6, 8, 10, 12] if not ragged else [0, 3, 4, 8, 10, 14, 15])
    k = 4
    values, rows, labels = m.nearest_exemplars(bnk, k)
    assert values.shape == rows.shape == labels.shape == (R, k) and rows.dtype == labels.dtype == torch.int64
    X = bnk.cpu()
    assert N.general_mismatch((values, rows.to(torch.int32)), X, X, k) is None
    s = X.double() @ X.double().t()
    own = s.diagonal()
    others = s.clone().fill_diagonal_(-1.0).max(1).values
    clear = (own - others > N.margin(X.shape[1], float(s.max()))).nonzero().flatten().tolist()
    assert all(int(rows[r, 0]) == r for r in clear if r not in (lo, hi))
    # the duplicate: two rows of one content score alike for every query; the lower row comes first
    for q in (lo, hi):
        got = rows[q].tolist()
        assert lo in got and hi in got and got.index(hi) == got.index(lo) + 1 and float(values[q, got.index(lo)]) == float(values[q, got.index(hi)])
    assert torch.equal(labels.cpu(), torch.searchsorted(starts[1:], rows.cpu(), right=True))
    # the per-class form equals the whole-bank call on that class's rows alone, offset by the class's start
    for c in range(6):
        a, e = int(starts[c]), int(starts[c + 1])
        n = min(k, e - a)
        v1, r1, l1 = m.nearest_exemplars(bnk, k, classes=torch.full((R,), c, dtype=torch.int64))
        assert v1.shape == (R, 1, k)
        v0, r0 = runtime.nearest_rows(bnk, bnk[a:e], n)
        assert torch.equal(r1[:, 0, :n], r0.long() + a) and torch.equal(v1[:, 0, :n], v0) and bool((l1[:, 0, :n] == c).all())
        assert bool((r1[:, 0, n:] == -1).all()) and bool((l1[:, 0, n:] == -1).all()) and bool(torch.isinf(v1[:, 0, n:]).all())
    # several classes per query in one launch
    cls = torch.stack([torch.arange(R) % 6, (torch.arange(R) + 2) % 6], 1)
    v2, r2, l2 = m.nearest_exemplars(bnk, 2, classes=cls.cuda())
    for j in range(2):
        v1, r1, _ = m.nearest_exemplars(bnk, 2, classes=cls[:, j].contiguous())
        assert torch.equal(v2[:, j], v1[:, 0]) and torch.equal(r2[:, j], r1[:, 0])


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_generated_store_and_loaded_bank_agree(ragged, clip, tmp_path):
    gen = _scratch(range(6), ragged, "", clip)
    gen.save_bank(str(tmp_path / bank.BANK_FILE))
    m = _model([8, 7], ragged)
    m.load_bank(str(tmp_path / bank.BANK_FILE))
    assert m.eval_row_labels is not None and (gen.eval_row_labels is None) == (not ragged)
    feats = gen.engine.encode_image(QUERIES[0], normalize=True)
    feats2 = m.engine.encode_image(QUERIES[0], normalize=True)
    assert torch.equal(feats, feats2)
    for classes in (None, torch.tensor([[0, 5], [1, 1], [2, 3], [4, 0], [5, 2]])):
        a, b = gen.nearest_exemplars(feats, 3, classes), m.nearest_exemplars(feats2, 3, classes)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    # an image batch is encoded by the call itself
    c = gen.nearest_exemplars(QUERIES[0], 3)
    assert all(torch.equal(x, y) for x, y in zip(c, gen.nearest_exemplars(feats, 3)))


def test_predict_explained_is_predict_topk_plus_neighbours(clip):
    m = _scratch(range(6), True, "", clip)
    for q in QUERIES:
        want = m.predict_topk(q, 3)
        values, indices, sims, rows = m.predict_explained(q, 3, 2)
        assert torch.equal(values, want[0]) and torch.equal(indices, want[1])
        feats = m.engine.encode_image(q, normalize=True)
        v, r, _ = m.nearest_exemplars(feats, 2, classes=indices)
        assert torch.equal(sims, v) and torch.equal(rows, r) and sims.shape == (q.shape[0], 3, 2)


def test_refusals(clip, tmp_path):
    m = _scratch(range(6), False, str(tmp_path), clip)
    m.wait_files()
    feats = m.engine.encode_image(QUERIES[0], normalize=True)
    with pytest.raises(ValueError, match=r"nearest_exemplars: k must be an integer in \[1, 32\], got 33"):
        m.nearest_exemplars(feats, 33)
    with pytest.raises(ValueError, match="nearest_exemplars: k = 13 exceeds the bank's 12 exemplar rows"):
        m.nearest_exemplars(feats, 13)
    with pytest.raises(ValueError, match="nearest_exemplars: classes must be class labels in"):
        m.nearest_exemplars(feats, 2, classes=torch.full((5,), 6, dtype=torch.int64))
    with pytest.raises(ValueError, match="nearest_exemplars: classes must be int64"):
        m.nearest_exemplars(feats, 2, classes=torch.zeros((4,), dtype=torch.int64))
    with pytest.raises(ValueError, match="predict_explained: n must be an integer"):
        m.predict_explained(QUERIES[0], 3, 0)
    m.load_classifiers(str(tmp_path / "mm_classifiers.pt"))
    with pytest.raises(ValueError, match="nearest_exemplars: the model holds no exemplar features"):
        m.nearest_exemplars(feats, 2)
    with pytest.raises(ValueError, match="predict_explained: the model holds no exemplar features"):
        m.predict_explained(QUERIES[0], 3, 2)


class _SmallLoader:
    """One class per batch, S images each, at the `small` model's resolution."""

    def __init__(self, spec, classes):
        self.spec, self.classes = spec, list(classes)

    def __iter__(self):
        for k, u in enumerate(self.classes):
            img = torch.from_numpy(synth.images(S, self.spec.image_resolution, 1000 + u, np.full(S, u), 0.6))
            yield {"img": img, "label": torch.full((S,), k, dtype=torch.long)}

    def __len__(self):
        return len(self.classes)


def test_small_spec_width_256():
    """The `small` model's embedding width (256): a generated uniform store queried with its own rows, whole bank and per class."""
    from ovmr_amd import modules
    spec = synth.SPECS["small"]
    clip = modules.CLIPModel({k: torch.from_numpy(v) for k, v in synth.clip_state_dict(spec, SEED, jitter=True).items()}, spec)
    cfg = modules.make_cfg(n_ctx=2, num_shots=S, test_batch_size=S)
    pl = {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, 2, SEED, True).items()}
    m = modules.CustomCLIP(cfg, _rows(list(range(4))), clip, prompt_learner_state=pl, reserve=(64, 64, 256), stream_text=True)
    m.forward_prompt(_SmallLoader(spec, range(4)))
    bnk, _ = m._exemplar_bank()
    assert bnk.shape == (4 * S, 256)
    values, rows, labels = m.nearest_exemplars(bnk, 3)
    X = bnk.cpu()
    assert N.general_mismatch((values, rows.to(torch.int32)), X, X, 3) is None and torch.equal(labels, rows // S)
    v1, r1, l1 = m.nearest_exemplars(bnk, S, classes=labels[:, 0].contiguous())
    assert bool((l1 == labels[:, :1, None]).all()) and bool((r1 // S == labels[:, :1, None]).all())


def test_runner_predict_nearest(golden, tmp_path, monkeypatch):
    """--save-bank with --predict --nearest in the generating run, then --bank alone with and without --nearest: predictions.csv is the same
    bytes in all three, neighbours.csv holds what predict_explained returned, row by row, with the bank's exemplar paths."""
    from PIL import Image
    from ovmr_amd import checkpoint, cli, modules
    from test_zeroshot_cpu import zsclip_bpe
    R, k, n = SPEC.image_resolution, 3, 3
    old, pics = tmp_path / "old", tmp_path / "pics"
    (old / "classnames.txt").parent.mkdir()
    (old / "classnames.txt").write_text(_class_folders(old / "train", 0, OLD, np.random.default_rng(3)))
    pics.mkdir()
    rng = np.random.default_rng(5)
    for i in range(7):
        base = np.full((36 + i, 50 - i, 3), 33 * i + 20, dtype=np.int32) + rng.integers(-20, 20, (36 + i, 50 - i, 3))
        Image.fromarray(base.clip(0, 255).astype(np.uint8)).save(pics / f"img{i}.png")
    bpe = str(tmp_path / "bpe.txt.gz")
    zsclip_bpe(bpe, golden)
    torch.save({k_: torch.from_numpy(v) for k_, v in synth.clip_state_dict(SPEC, SEED, jitter=True).items()}, tmp_path / "clip.pt")
    checkpoint.save_prompt_learner_state(_pl_state(), str(tmp_path / "ckpt"), 30)
    common = ["--seed", "1", "--trainer", "MM_CLS_OP", "--eval-only", "--clip-weights", str(tmp_path / "clip.pt"), "--bpe-path", bpe,
              "--model-dir", str(tmp_path / "ckpt"), "--load-epoch", "30", "--eval_mode", "fusion", "--eval_tau", "10", "--n_ctx", "2",
              "--workers", "2", "--predict", str(pics), "--topk", str(k)]
    opts = ["DATASET.NAME", "ImageNet", "INPUT.SIZE", f"({R}, {R})", "DATALOADER.TEST.BATCH_SIZE", str(S), "DATASET.NUM_SHOTS", str(S)]
    seen = []
    real = modules.CustomCLIP.predict_explained

    def recording(self, *a, **kw):
        out = real(self, *a, **kw)
        seen.append(tuple(t.cpu() for t in out))
        return out

    monkeypatch.setattr(modules.CustomCLIP, "predict_explained", recording)
    res = cli.main(common + ["--root", str(old), "--output-dir", str(tmp_path / "o_gen"), "--save-bank", "--nearest", str(n)] + opts)
    assert sorted(p.name for p in (tmp_path / "o_gen").iterdir()) == ["mm_classifiers.pt", "neighbours.csv", "predictions.csv", "reference_bank.pt",
                                                                       "visual_tokens.pt"]
    bank_file = str(tmp_path / "o_gen" / "reference_bank.pt")
    saved = bank.read(bank_file)
    gen_seen, seen[:] = list(seen), []
    plain = cli.main(common + ["--bank", bank_file, "--output-dir", str(tmp_path / "o_plain")] + opts)
    assert not seen and sorted(p.name for p in (tmp_path / "o_plain").iterdir()) == ["predictions.csv"]
    res2 = cli.main(common + ["--bank", bank_file, "--output-dir", str(tmp_path / "o_near"), "--nearest", str(n)] + opts)
    assert sorted(p.name for p in (tmp_path / "o_near").iterdir()) == ["neighbours.csv", "predictions.csv"]
    want = (tmp_path / "o_plain" / "predictions.csv").read_bytes()
    assert (tmp_path / "o_near" / "predictions.csv").read_bytes() == want == (tmp_path / "o_gen" / "predictions.csv").read_bytes()
    assert res2["predictions"] == plain["predictions"] == res["predictions"]
    assert (tmp_path / "o_near" / "neighbours.csv").read_bytes() == (tmp_path / "o_gen" / "neighbours.csv").read_bytes()
    for got, batches in ((res, gen_seen), (res2, seen)):
        indices, sims, rows = (torch.cat([b[i] for b in batches]) for i in (1, 2, 3))
        assert indices.shape == (7, k) and rows.shape == (7, k, n) and int((rows < 0).sum()) == 7 * k * (n - S)   # S = 2 exemplars per class: one -1 each
    lines = list(csv.reader(open(tmp_path / "o_near" / "neighbours.csv")))
    assert lines[0] == cli.NEIGHBOUR_COLUMNS and len(lines) == 1 + 7 * k * S
    images = sorted(str(p) for p in pics.iterdir())
    it = iter(lines[1:])
    for i, image in enumerate(images):
        for rank in range(k):
            c = int(indices[i, rank])
            for j in range(n):
                row = int(rows[i, rank, j])
                if row < 0:
                    assert j >= S and sims[i, rank, j] == -np.inf
                    continue
                assert next(it) == [image, str(rank), str(c), OLD[c], str(j), str(row), saved["exemplar_paths"][row], repr(float(sims[i, rank, j]))]
                assert c * S <= row < (c + 1) * S
    # the refusals: one line each, before anything is loaded
    for extra, msg in ((["--trainer", "ZeroshotCLIP"], "has no exemplars to search"), (["--classifiers", str(tmp_path / "o_gen" / "mm_classifiers.pt")], "holds no exemplar features"),
                       (["--nearest", "33"], r"N must lie in \[1, 32\]")):
        with pytest.raises(SystemExit, match=msg):
            cli.main(common + ["--root", str(old), "--output-dir", str(tmp_path / "o_no"), "--nearest", str(n)] + extra + opts)
