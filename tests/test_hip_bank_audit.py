"""CustomCLIP.audit_bank and the runner's --audit-bank on the device, against audit_cases.py:

  a. exact-operand features installed into the exemplar store of a generated `tiny` model, uniform and ragged: every field equals
     audit_cases.expected_audit -- a copy inside a class, a copy across two classes, a row whose best match lies in another class, equal
     best scores on both sides (not suspect; the lower row is the duplicate), classes of one image, `classes=` subsets, dup_threshold
     exactly at a planted dyadic score and one fp16 step above it, every batch size;
  b. the model's own generated features: a planted copy is reported at the default threshold (after the CPU's fp64 scores say that it
     wins by more than the margin), the lists hold by margin;
  c. save_bank -> load_bank -> audit_bank gives equal tensors;
  d. refusals, one line each;
  e. the runner: --bank FILE --audit-bank 3 writes the three files, decodes nothing, and leaves predictions.csv of a combined --predict
     byte-identical to the run without the flag.
Needs an MI355X: run with `pytest -m gpu`.
"""
import csv

import numpy as np
import pytest
import torch

import audit_cases as A
import nearest_cases as N
from ovmr_amd import bank, synth
from test_bank_cpu import RAGGED
from test_hip_bank import OLD, S, SEED, SPEC, _class_folders, _clip, _model, _pl_state, _scratch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clip():
    return _clip()


def _lens(ragged, C=8):
    return tuple(RAGGED[:C]) if ragged else (S,) * C


def _install(m, X):
    """The exemplar store takes the rows of X (label order: the generation's loaders go class after class), in place."""
    store = m.eval_feat4cls
    store.view(-1, store.shape[-1]).copy_(X.to(store.device))
    m.__dict__.pop("_nearest_bank", None)


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_exact_features_every_field(ragged, clip):
    m = _scratch(range(8), ragged, "", clip)
    lens = _lens(ragged)
    X, starts, s16 = A.audit_bank_case(SPEC.embed_dim, lens)
    _install(m, X)
    bnk, dstarts = m._exemplar_bank()
    assert dstarts.tolist() == starts and torch.equal(bnk.cpu(), X)
    rows = A.plant_rows(lens)
    for k in (1, 3, 5):
        want = A.expected_audit(s16, starts, k)
        got = m.audit_bank(k)
        msg = A.audit_mismatch(got, want)
        assert msg is None, f"k = {k}: {msg}"
        assert all(t.is_cuda for t in got.values())
    want = A.expected_audit(s16, starts, 3)
    dup, sus = want["duplicate_of"].tolist(), want["suspect"].tolist()
    a, b = rows["copy"]
    assert dup[a] == b and dup[b] == a and not sus[a] and not sus[b], "a copy inside a class"
    a, b = rows["cross"]
    assert dup[a] == b and dup[b] == a and sus[a] and sus[b], "a copy across two classes"
    a, b = rows["near"]
    assert sus[b] and dup[b] == -1 and float(want["out_sim"][b, 0]) == A.NEAR and int(want["out_row"][b, 0]) == a, "the best match lies in another class"
    a, b, c = rows["equal_in"]
    assert not sus[a] and not sus[b] and dup[a] == b and dup[b] == a and float(want["in_sim"][a, 0]) == float(want["out_sim"][a, 0]) == 1.0
    a, b, c = rows["equal_out"]
    assert c < a and not sus[a] and dup[a] == c and dup[b] == c, "equal scores: the lower row, out of class, is the duplicate"
    if ragged:
        ones = [c for c, n in enumerate(lens) if n == 1]
        assert ones and all(int(want["class_suspects"][c]) == 0 and int(want["in_row"][starts[c], 0]) == -1 for c in ones), "a class of one image"
    # classes= restricts the audited rows; the search still sees the whole bank
    for classes in ([2], [7, 0, 3], torch.tensor([4, 4, 1]), []):
        msg = A.audit_mismatch(m.audit_bank(3, classes=classes), A.expected_audit(s16, starts, 3, [int(c) for c in classes]))
        assert msg is None, f"classes = {classes}: {msg}"
    # the threshold: >= holds exactly at the planted score, not one fp16 step above it
    at, above = A.expected_audit(s16, starts, 3, dup_threshold=A.NEAR), A.expected_audit(s16, starts, 3, dup_threshold=A.NEAR + 2.0 ** -11)
    assert int((at["duplicate_of"] >= 0).sum()) == int((above["duplicate_of"] >= 0).sum()) + 2
    assert A.audit_mismatch(m.audit_bank(3, dup_threshold=A.NEAR), at) is None
    assert A.audit_mismatch(m.audit_bank(3, dup_threshold=A.NEAR + 2.0 ** -11), above) is None
    for batch in (1, 5, 7, 4096):
        assert A.audit_mismatch(m.audit_bank(3, batch=batch), want) is None, f"batch = {batch}"


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_generated_features_by_margin_and_a_planted_copy(ragged, clip):
    m = _scratch(range(6), ragged, "", clip)
    bnk, starts = m._exemplar_bank()
    X = bnk.cpu().clone()
    starts = starts.tolist()
    R, k = X.shape[0], 3
    lo, hi = 1, R - 2                                             # two classes, far apart
    X[hi] = X[lo]
    s = X.double() @ X.double().t()
    margin = N.margin(X.shape[1], float(s.abs().max()))
    others = s[lo].clone()
    others[[lo, hi]] = -2.0
    assert float(s[lo, hi]) - float(others.max()) > margin, "the plant must win by more than the margin"
    assert float(s[lo, hi]) > 0.9990, "an fp16 L2-normalised row against its copy"
    _install(m, X)
    got = m.audit_bank(k)
    assert int(got["duplicate_of"][lo]) == hi and int(got["duplicate_of"][hi]) == lo
    assert bool(got["suspect"][lo]) and bool(got["suspect"][hi])
    labels = got["labels"].cpu()
    own = torch.tensor([[starts[int(c)], starts[int(c) + 1]] for c in labels], dtype=torch.int32)
    me = torch.stack([torch.arange(R), torch.arange(R) + 1], 1).to(torch.int32)
    msg = A.margin_mismatch((got["in_sim"], got["in_row"].to(torch.int32)), X, X, k, own, me)
    assert msg is None, f"inside the class: {msg}"
    msg = A.margin_mismatch((got["out_sim"], got["out_row"].to(torch.int32)), X, X, k, None, own)
    assert msg is None, f"outside the class: {msg}"
    assert torch.equal(got["rows"].cpu(), torch.arange(R)) and torch.equal(labels, torch.searchsorted(torch.tensor(starts[1:]), torch.arange(R), right=True))


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_saved_and_loaded_bank_audit_alike(ragged, clip, tmp_path):
    gen = _scratch(range(8), ragged, "", clip)
    X, starts, s16 = A.audit_bank_case(SPEC.embed_dim, _lens(ragged))
    _install(gen, X)
    gen.save_bank(str(tmp_path / bank.BANK_FILE))
    m = _model([8, 7], ragged)
    m.load_bank(str(tmp_path / bank.BANK_FILE))
    a, b = gen.audit_bank(4), m.audit_bank(4)
    assert set(a) == set(b) == set(A.AUDIT_FIELDS)
    for f in A.AUDIT_FIELDS:
        assert torch.equal(a[f], b[f]), f
    assert A.audit_mismatch(b, A.expected_audit(s16, starts, 4)) is None


def test_refusals(clip, tmp_path):
    m = _scratch(range(6), False, str(tmp_path), clip)
    m.wait_files()
    for k, msg in ((0, r"audit_bank: k must be an integer in \[1, 32\], got 0"), (33, r"audit_bank: k must be an integer in \[1, 32\], got 33"),
                   (2.0, "audit_bank: k must be an integer"), (13, "audit_bank: k = 13 exceeds the bank's 12 exemplar rows")):
        with pytest.raises(ValueError, match=msg) as err:
            m.audit_bank(k)
        assert "\n" not in str(err.value)
    with pytest.raises(ValueError, match=r"audit_bank: classes must be integer labels in \[0, 6\)"):
        m.audit_bank(3, classes=[6])
    with pytest.raises(ValueError, match="audit_bank: batch must be a positive integer"):
        m.audit_bank(3, batch=0)
    with pytest.raises(ValueError, match="audit_bank: dup_threshold must be a number"):
        m.audit_bank(3, dup_threshold=float("nan"))
    m.load_classifiers(str(tmp_path / "mm_classifiers.pt"))
    with pytest.raises(ValueError, match="audit_bank: the model holds no exemplar features") as err:
        m.audit_bank(3)
    assert "\n" not in str(err.value)


def test_runner_audit_bank(golden, tmp_path, monkeypatch):
    """--save-bank in a generating run; then --bank FILE --audit-bank 3 alone (no --root, no --predict: three files, nothing decoded), and
    with --predict next to the run without the flag: predictions.csv is the same bytes."""
    from PIL import Image
    from ovmr_amd import checkpoint, cli, modules
    from test_zeroshot_cpu import zsclip_bpe
    R, k = SPEC.image_resolution, 3
    old, pics = tmp_path / "old", tmp_path / "pics"
    (old / "classnames.txt").parent.mkdir()
    (old / "classnames.txt").write_text(_class_folders(old / "train", 0, OLD, np.random.default_rng(3)))
    pics.mkdir()
    rng = np.random.default_rng(5)
    for i in range(5):
        base = np.full((36 + i, 50 - i, 3), 33 * i + 20, dtype=np.int32) + rng.integers(-20, 20, (36 + i, 50 - i, 3))
        Image.fromarray(base.clip(0, 255).astype(np.uint8)).save(pics / f"img{i}.png")
    bpe = str(tmp_path / "bpe.txt.gz")
    zsclip_bpe(bpe, golden)
    torch.save({k_: torch.from_numpy(v) for k_, v in synth.clip_state_dict(SPEC, SEED, jitter=True).items()}, tmp_path / "clip.pt")
    checkpoint.save_prompt_learner_state(_pl_state(), str(tmp_path / "ckpt"), 30)
    base = ["--seed", "1", "--trainer", "MM_CLS_OP", "--eval-only", "--clip-weights", str(tmp_path / "clip.pt"), "--bpe-path", bpe,
            "--model-dir", str(tmp_path / "ckpt"), "--load-epoch", "30", "--eval_mode", "fusion", "--eval_tau", "10", "--n_ctx", "2", "--workers", "2"]
    predict = ["--predict", str(pics), "--topk", str(k)]
    opts = ["DATASET.NAME", "ImageNet", "INPUT.SIZE", f"({R}, {R})", "DATALOADER.TEST.BATCH_SIZE", str(S), "DATASET.NUM_SHOTS", str(S)]
    seen = []
    real = modules.CustomCLIP.audit_bank

    def recording(self, *a, **kw):
        out = real(self, *a, **kw)
        seen.append({f: t.cpu() for f, t in out.items()})
        return out

    monkeypatch.setattr(modules.CustomCLIP, "audit_bank", recording)
    # the generating run audits the state it ends with
    res = cli.main(base + predict + ["--root", str(old), "--output-dir", str(tmp_path / "o_gen"), "--save-bank", "--audit-bank", "3"] + opts)
    assert sorted(p.name for p in (tmp_path / "o_gen").iterdir()) == sorted(["mm_classifiers.pt", "predictions.csv", "reference_bank.pt", "visual_tokens.pt",
                                                                              *cli.AUDIT_FILES])
    bank_file = str(tmp_path / "o_gen" / "reference_bank.pt")
    saved = bank.read(bank_file)
    # the bank alone: no --root, no --predict; nothing is decoded
    listed = []
    factory = cli._loader_factory

    def recording_factory(*a, **kw):
        make = factory(*a, **kw)
        return lambda items, *b, **kw2: (listed.append(len(items)), make(items, *b, **kw2))[1]

    def no_splits(*a, **kw):
        raise AssertionError("the audit of a bank lists no data set")

    monkeypatch.setattr(cli, "_loader_factory", recording_factory)
    monkeypatch.setattr(cli, "build_splits", no_splits)
    alone = cli.main(base + ["--bank", bank_file, "--output-dir", str(tmp_path / "o_audit"), "--audit-bank", "3"] + opts)
    assert sorted(p.name for p in (tmp_path / "o_audit").iterdir()) == sorted(cli.AUDIT_FILES) and listed == [0], "no image is handed to a loader"
    assert "predictions" not in alone and not any(key.startswith("pipeline_") for key in alone) and alone["classnames"] == OLD
    for name in cli.AUDIT_FILES:
        assert (tmp_path / "o_audit" / name).read_bytes() == (tmp_path / "o_gen" / name).read_bytes(), name
    audit = seen[-1]
    n_rows = len(OLD) * S
    assert audit["rows"].tolist() == list(range(n_rows)) and len(seen) == 2 and all(torch.equal(seen[0][f], audit[f]) for f in audit)
    lines = list(csv.reader(open(tmp_path / "o_audit" / "bank_audit.csv")))
    assert lines[0] == cli.AUDIT_COLUMNS and len(lines) == 1 + n_rows
    for r, line in enumerate(lines[1:]):
        c, o = r // S, int(audit["out_label"][r, 0])
        assert line == [str(r), str(c), OLD[c], saved["exemplar_paths"][r], str(int(audit["in_row"][r, 0])), repr(float(audit["in_sim"][r, 0])),
                        str(int(audit["out_row"][r, 0])), str(o), OLD[o], repr(float(audit["out_sim"][r, 0])), str(int(audit["suspect"][r])),
                        str(int(audit["duplicate_of"][r]))]
    assert alone["bank_audit"]["exemplars"][0][:4] == (0, 0, OLD[0], saved["exemplar_paths"][0])
    nb = list(csv.reader(open(tmp_path / "o_audit" / "bank_audit_neighbours.csv")))
    # S = 2 images per class: one class-mate each, three neighbours outside
    assert nb[0] == cli.AUDIT_NEIGHBOUR_COLUMNS and len(nb) == 1 + n_rows * (1 + 3)
    assert nb[1] == ["0", "in", "0", str(int(audit["in_row"][0, 0])), "0", repr(float(audit["in_sim"][0, 0]))]
    assert nb[2] == ["0", "out", "0", str(int(audit["out_row"][0, 0])), str(int(audit["out_label"][0, 0])), repr(float(audit["out_sim"][0, 0]))]
    cl = list(csv.reader(open(tmp_path / "o_audit" / "bank_audit_classes.csv")))
    assert cl[0] == cli.AUDIT_CLASS_COLUMNS
    assert cl[1:] == [[str(c), OLD[c], str(S), str(int(audit["class_suspects"][c])), str(int(audit["class_duplicates"][c]))] for c in range(len(OLD))]
    monkeypatch.setattr(cli, "_loader_factory", factory)
    # next to --predict: predictions.csv is what the run without the flag writes
    plain = cli.main(base + predict + ["--bank", bank_file, "--output-dir", str(tmp_path / "o_plain")] + opts)
    both = cli.main(base + predict + ["--bank", bank_file, "--output-dir", str(tmp_path / "o_both"), "--audit-bank", "3", "--dup-threshold", "0.5"] + opts)
    assert sorted(p.name for p in (tmp_path / "o_both").iterdir()) == sorted(["predictions.csv", *cli.AUDIT_FILES])
    want = (tmp_path / "o_plain" / "predictions.csv").read_bytes()
    assert (tmp_path / "o_both" / "predictions.csv").read_bytes() == want == (tmp_path / "o_gen" / "predictions.csv").read_bytes()
    assert both["predictions"] == plain["predictions"] == res["predictions"] and "bank_audit" not in plain
    assert (tmp_path / "o_both" / "bank_audit_neighbours.csv").read_bytes() == (tmp_path / "o_audit" / "bank_audit_neighbours.csv").read_bytes()
    low = seen[-1]
    assert int((low["duplicate_of"] >= 0).sum()) >= int((audit["duplicate_of"] >= 0).sum())
    assert torch.equal(low["duplicate_of"] >= 0, torch.maximum(low["in_sim"][:, 0], low["out_sim"][:, 0]) >= 0.5)
    # the refusals: one line each, before anything is loaded
    for extra, msg in ((["--trainer", "ZeroshotCLIP", "--audit-bank", "3"], "has no exemplars to audit"),
                       (predict + ["--classifiers", str(tmp_path / "o_gen" / "mm_classifiers.pt"), "--audit-bank", "3"], "holds no exemplar features"),
                       (["--audit-bank", "33"], r"K must lie in \[1, 32\]"), (["--dup-threshold", "0.9"], "--dup-threshold T belongs to --audit-bank")):
        with pytest.raises(SystemExit, match=msg) as err:
            cli.main(base + ["--root", str(old), "--output-dir", str(tmp_path / "o_no")] + extra + opts)
        assert "\n" not in str(err.value)
