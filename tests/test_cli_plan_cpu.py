"""The runner's refusals, pinned: which one wins when a command line breaks several rules at once, and the job plan on its own.

TABLE holds command lines that break two or more rules, each with the message `cli.main` exits with.  The texts were recorded from the
runner before its `main` was split into a plan and stages, so the table holds the ORDER of the refusals as well as their words.  Every
case ends before torch or the CLIP weights are touched: `--clip-weights` names a file that does not exist, `--root` a folder that does
not, and `_no_library` turns a look at either into an AssertionError.  No GPU, no weights."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MM = ["--eval-only", "--trainer", "MM_CLS_OP"]
ZS = ["--eval-only", "--trainer", "ZeroshotCLIP", "DATASET.NAME", "Caltech101"]
ZS2 = ["--eval-only", "--trainer", "ZeroshotCLIP2", "DATASET.NAME", "Caltech101"]
ONE_OF = ("only `--eval-only --trainer MM_CLS_OP` (classifier generation / evaluation) and `--eval-only --trainer ZeroshotCLIP | ZeroshotCLIP2` "
          "(zero-shot evaluation) are on the hot path")
NEEDS_BANK = "--add-classes / --replace-classes / --remove-classes edit a reference bank: give --bank FILE"
ZS_BANK = ("--bank / --save-bank: --trainer ZeroshotCLIP has no generated vocabulary to bank (MM_CLS_OP only; a zero-shot vocabulary is a text "
           "call away)")
BANK_ONE_PROCESS = "--bank / --save-bank run in one process: a sharded rank holds only its own classes' exemplar features"
BANK_SAVE = "--save-bank belongs to a generation job: a --bank run writes OUTPUT_DIR/reference_bank.pt whenever it edits"
BANK_CLF = "--bank holds the classifiers already: not together with --classifiers"
ONE_OF_TWO = "--retrieve searches a pool by class, --predict ranks the classes of every image: one of the two per run"
RETRIEVE_ALL = "--retrieve searches under ONE mode: --eval_mode all belongs to the test pass (fusion, text, vision or multimodal here)"
PREDICT_ALL = "--predict ranks the classes under ONE mode: --eval_mode all belongs to the test pass (fusion, text, vision or multimodal here)"
TOPK_RETRIEVE = "--topk K belongs to --predict PATH (--retrieve takes --per-class M and --within-top K)"
CURVES_OF = "--score-curves belongs to the test pass: {} reads unlabelled images, a score has no label to be held against"
RANGE_BELONGS = "--score-range LO HI belongs to --score-curves [BINS]: the range the score histograms of the test pass cover"
NEAREST_BELONGS = "--nearest N belongs to --predict PATH: the nearest exemplars of every predicted class"
NO_EXEMPLARS = "(MM_CLS_OP only; a zero-shot trainer's classifier rows are text features)"
NO_FEATURES = "holds no exemplar features (generate in this run, or start from --bank)"
DUP_BELONGS = "--dup-threshold T belongs to --audit-bank [K]: the similarity from which a neighbour counts as a duplicate"
AUDIT_ONE_PROCESS = "--audit-bank runs in one process: a sharded rank holds only its own classes' exemplar features"
PREDICT_ONE_PROCESS = "--predict runs in one process: sharding the prediction pass over ranks is not implemented"
NOTHING_TO_COUNT = "{} belongs to the test pass: {} unlabelled images, there is nothing to count"
BELONG_TO_PREDICT = "--topk / --classifiers belong to --predict PATH (the test pass takes TEST.TOPK)"
SHOTS = "DATASET.NUM_SHOTS must be >= 1: the eval-set loader draws NUM_SHOTS rows per class (data_manager.py:157-170)"
EXTENSIONS = ".jpg, .jpeg, .png, .bmp, .gif, .ppm, .pgm, .tif, .tiff, .webp"

# (id, WORLD_SIZE, arguments, message); {pics} a folder with one image, {empty} one without, {bank} / {clf} files that exist, {gone} a
# path below which nothing exists.  The flags stand in front of the KEY VALUE opts, which end a command line
TABLE = [
    # not this runner's job at all
    ("trainer-unknown+edit", 1, ["--add-classes", "{gone}/x", "--eval-only", "--trainer", "CoOp"], ONE_OF),
    ("no-eval-only+bank+save", 1, ["--bank", "{bank}", "--save-bank", "--trainer", "MM_CLS_OP"], ONE_OF),
    # the edit flags need a bank
    ("add+save-bank/zs", 1, ["--add-classes", "{gone}/x", "--save-bank"] + ZS, NEEDS_BANK),
    ("remove+save-bank/world2", 2, ["--remove-classes", "a", "--save-bank"] + MM, NEEDS_BANK),
    ("replace+classifiers", 1, ["--replace-classes", "{gone}/x", "--classifiers", "{clf}"] + MM, NEEDS_BANK),
    ("add+predict+nearest", 1, ["--add-classes", "{gone}/x", "--predict", "{pics}", "--nearest", "2"] + MM, NEEDS_BANK),
    ("remove+retrieve+topk", 1, ["--remove-classes", "a", "b", "--retrieve", "{pics}", "--topk", "3"] + MM, NEEDS_BANK),
    ("add+audit+score-curves", 1, ["--add-classes", "{gone}/x", "--audit-bank", "--score-curves"] + MM, NEEDS_BANK),
    # a zero-shot trainer against the bank flags
    ("zs+bank-missing/world2", 2, ["--bank", "{gone}/bank.pt"] + ZS, ZS_BANK),
    ("zs+save-bank+audit", 1, ["--save-bank", "--audit-bank"] + ZS, ZS_BANK),
    ("zs+bank+save-bank+classifiers", 1, ["--bank", "{bank}", "--save-bank", "--classifiers", "{clf}"] + ZS, ZS_BANK),
    ("zs2+bank+edit", 1, ["--bank", "{bank}", "--remove-classes", "a"] + ZS2, ZS_BANK.replace("ZeroshotCLIP", "ZeroshotCLIP2")),
    # WORLD_SIZE 2 against the bank
    ("bank+save-bank/world2", 2, ["--bank", "{bank}", "--save-bank"] + MM, BANK_ONE_PROCESS),
    ("bank+audit/world2", 2, ["--bank", "{bank}", "--audit-bank"] + MM, BANK_ONE_PROCESS),
    ("save-bank+predict/world2", 2, ["--save-bank", "--predict", "{pics}"] + MM, BANK_ONE_PROCESS),
    ("bank-missing+retrieve/world2", 2, ["--bank", "{gone}/bank.pt", "--retrieve", "{pics}"] + MM, BANK_ONE_PROCESS),
    # the bank flags among themselves
    ("bank+save-bank+classifiers", 1, ["--bank", "{bank}", "--save-bank", "--classifiers", "{clf}"] + MM, BANK_SAVE),
    ("bank+save-bank+add-missing", 1, ["--bank", "{bank}", "--add-classes", "{gone}/x", "--save-bank"] + MM, BANK_SAVE),
    ("bank-missing+classifiers+predict", 1, ["--bank", "{gone}/bank.pt", "--classifiers", "{clf}", "--predict", "{pics}"] + MM, BANK_CLF),
    ("bank+replace+classifiers", 1, ["--bank", "{bank}", "--replace-classes", "{gone}/x", "--classifiers", "{clf}"] + MM, BANK_CLF),
    ("bank-missing+retrieve+predict", 1, ["--bank", "{gone}/bank.pt", "--retrieve", "{pics}", "--predict", "{pics}"] + MM,
     "--bank '{gone}/bank.pt': no such file"),
    ("bank-missing+per-class", 1, ["--bank", "{gone}/bank.pt", "--per-class", "3"] + MM, "--bank '{gone}/bank.pt': no such file"),
    ("bank-missing+nearest+audit0", 1, ["--bank", "{gone}/bank.pt", "--nearest", "2", "--audit-bank", "0"] + MM,
     "--bank '{gone}/bank.pt': no such file"),
    # --retrieve and its flags
    ("per-class+score-range", 1, ["--per-class", "3", "--score-range", "0", "1"] + MM,
     "--per-class M belongs to --retrieve PATH: the search of an image pool by class"),
    ("per-class+within-top", 1, ["--per-class", "3", "--within-top", "2"] + MM,
     "--per-class M belongs to --retrieve PATH: the search of an image pool by class"),
    ("within-top+nearest", 1, ["--within-top", "3", "--nearest", "2"] + MM,
     "--within-top K belongs to --retrieve PATH: the search of an image pool by class"),
    ("per-class+predict+topk0", 1, ["--per-class", "3", "--predict", "{pics}", "--topk", "0"] + MM,
     "--per-class M belongs to --retrieve PATH: the search of an image pool by class"),
    ("retrieve+predict+score-curves", 1, ["--retrieve", "{pics}", "--predict", "{pics}", "--score-curves"] + MM, ONE_OF_TWO),
    ("retrieve+predict+nearest/zs", 1, ["--retrieve", "{pics}", "--predict", "{pics}", "--nearest", "2"] + ZS, ONE_OF_TWO),
    ("retrieve+all+topk", 1, ["--retrieve", "{pics}", "--eval_mode", "all", "--topk", "3"] + MM, RETRIEVE_ALL),
    ("retrieve+all+topk/zs", 1, ["--retrieve", "{pics}", "--eval_mode", "all", "--topk", "3"] + ZS, TOPK_RETRIEVE),
    ("retrieve+per-class-result+per-class40", 1, ["--retrieve", "{pics}", "--per-class-result", "--per-class", "40"] + MM,
     NOTHING_TO_COUNT.format("--per-class-result", "--retrieve searches")),
    ("retrieve+confusion-matrix+topk", 1, ["--retrieve", "{pics}", "--confusion-matrix", "--topk", "3"] + MM,
     NOTHING_TO_COUNT.format("--confusion-matrix", "--retrieve searches")),
    ("retrieve+topk+per-class0", 1, ["--retrieve", "{pics}", "--topk", "3", "--per-class", "0"] + MM, TOPK_RETRIEVE),
    ("retrieve+per-class33+within-top0", 1, ["--retrieve", "{pics}", "--per-class", "33", "--within-top", "0"] + MM,
     "--per-class 33: M must lie in [1, 32]"),
    ("retrieve+within-top33+score-curves", 1, ["--retrieve", "{pics}", "--within-top", "33", "--score-curves"] + MM,
     "--within-top 33: K must lie in [1, min(32, number of classes)]"),
    ("bank+audit0+retrieve+per-class0", 1, ["--bank", "{bank}", "--audit-bank", "0", "--retrieve", "{pics}", "--per-class", "0"] + MM,
     "--per-class 0: M must lie in [1, 32]"),
    # --score-curves
    ("retrieve+score-curves+nearest", 1, ["--retrieve", "{pics}", "--score-curves", "--nearest", "2"] + MM, CURVES_OF.format("--retrieve")),
    ("predict+score-curves+per-class-result", 1, ["--predict", "{pics}", "--score-curves", "--per-class-result"] + MM,
     CURVES_OF.format("--predict")),
    ("score-range+nearest", 1, ["--score-range", "0", "1", "--nearest", "2"] + MM, RANGE_BELONGS),
    ("score-range+predict-missing", 1, ["--score-range", "0", "1", "--predict", "{gone}/pics"] + MM, RANGE_BELONGS),
    ("score-curves5000+dup-threshold", 1, ["--score-curves", "5000", "--dup-threshold", "0.9"] + MM,
     "--score-curves 5000: BINS must lie in [1, 4096]"),
    ("score-curves+nearest/zs", 1, ["--score-curves", "--nearest", "2"] + ZS,
     "--score-curves: --trainer ZeroshotCLIP returns logits, which have no natural range: give --score-range LO HI"),
    ("score-curves+range-reversed+audit40", 1, ["--score-curves", "--score-range", "1", "0", "--audit-bank", "40"] + MM,
     "--score-range 1.0 0.0: LO must lie below HI"),
    ("score-curves+range-nan+topk", 1, ["--score-curves", "--score-range", "nan", "1", "--topk", "3"] + MM,
     "--score-range nan 1.0: LO and HI must be finite"),
    ("score-curves+save-bank+topk", 1, ["--score-curves", "--save-bank", "--topk", "3"] + MM, BELONG_TO_PREDICT),
    # --nearest
    ("nearest+audit40", 1, ["--nearest", "2", "--audit-bank", "40"] + MM, NEAREST_BELONGS),
    ("nearest+retrieve", 1, ["--nearest", "2", "--retrieve", "{pics}"] + MM, NEAREST_BELONGS),
    ("nearest+predict+classifiers/zs", 1, ["--predict", "{pics}", "--nearest", "2", "--classifiers", "{clf}"] + ZS,
     "--nearest: --trainer ZeroshotCLIP has no exemplars to search " + NO_EXEMPLARS),
    ("nearest+predict+classifiers-missing+audit", 1, ["--predict", "{pics}", "--nearest", "2", "--classifiers", "{gone}/clf.pt", "--audit-bank"] + MM,
     "--nearest: --classifiers '{gone}/clf.pt' " + NO_FEATURES),
    ("nearest33+predict+audit0", 1, ["--predict", "{pics}", "--nearest", "33", "--audit-bank", "0"] + MM, "--nearest 33: N must lie in [1, 32]"),
    ("nearest0+predict/world2", 2, ["--predict", "{pics}", "--nearest", "0"] + MM, "--nearest 0: N must lie in [1, 32]"),
    # --audit-bank
    ("dup-threshold+topk", 1, ["--dup-threshold", "0.9", "--topk", "3"] + MM, DUP_BELONGS),
    ("dup-threshold+predict/world2", 2, ["--dup-threshold", "0.9", "--predict", "{pics}"] + MM, DUP_BELONGS),
    ("audit+predict+per-class-result/zs", 1, ["--audit-bank", "--predict", "{pics}", "--per-class-result"] + ZS,
     "--audit-bank: --trainer ZeroshotCLIP has no exemplars to audit " + NO_EXEMPLARS),
    ("audit+classifiers", 1, ["--audit-bank", "--classifiers", "{clf}"] + MM, "--audit-bank: --classifiers '{clf}' " + NO_FEATURES),
    ("audit33+dup-nan", 1, ["--audit-bank", "33", "--dup-threshold", "nan"] + MM, "--audit-bank 33: K must lie in [1, 32]"),
    ("audit+dup-nan/world2", 2, ["--audit-bank", "--dup-threshold", "nan"] + MM, "--dup-threshold nan: T must be a number"),
    ("audit+predict/world2", 2, ["--audit-bank", "--predict", "{pics}"] + MM, AUDIT_ONE_PROCESS),
    ("audit3+retrieve/world2", 2, ["--audit-bank", "3", "--retrieve", "{pics}"] + MM, AUDIT_ONE_PROCESS),
    # --predict
    ("predict+all+per-class-result", 1, ["--predict", "{pics}", "--eval_mode", "all", "--per-class-result"] + MM, PREDICT_ALL),
    ("predict+all+per-class-result/zs", 1, ["--predict", "{pics}", "--eval_mode", "all", "--per-class-result"] + ZS,
     NOTHING_TO_COUNT.format("--per-class-result", "--predict ranks")),
    ("predict+per-class-result+topk0/world2", 2, ["--predict", "{pics}", "--per-class-result", "--topk", "0"] + MM,
     NOTHING_TO_COUNT.format("--per-class-result", "--predict ranks")),
    ("predict+confusion-matrix/world2", 2, ["--predict", "{pics}", "--confusion-matrix"] + MM,
     NOTHING_TO_COUNT.format("--confusion-matrix", "--predict ranks")),
    ("predict+topk0/world2", 2, ["--predict", "{pics}", "--topk", "0"] + MM, PREDICT_ONE_PROCESS),
    ("predict-missing+classifiers/zs/world2", 2, ["--predict", "{gone}/pics", "--classifiers", "{clf}"] + ZS, PREDICT_ONE_PROCESS),
    ("predict-missing+topk33+classifiers-missing", 1, ["--predict", "{gone}/pics", "--topk", "33", "--classifiers", "{gone}/clf.pt"] + MM,
     "--topk 33: K must lie in [1, min(32, number of classes)]"),
    ("bank+predict-missing+topk40", 1, ["--bank", "{bank}", "--predict", "{gone}/pics", "--topk", "40"] + MM,
     "--topk 40: K must lie in [1, min(32, number of classes)]"),
    ("predict-missing+classifiers-missing/zs", 1, ["--predict", "{gone}/pics", "--classifiers", "{gone}/clf.pt"] + ZS,
     "--classifiers '{gone}/clf.pt': --trainer ZeroshotCLIP has no generated classifiers to load (MM_CLS_OP only)"),
    ("predict-missing+classifiers-missing", 1, ["--predict", "{gone}/pics", "--classifiers", "{gone}/clf.pt"] + MM,
     "--classifiers '{gone}/clf.pt': no such file"),
    ("save-bank+predict+classifiers-missing", 1, ["--save-bank", "--predict", "{pics}", "--classifiers", "{gone}/clf.pt"] + MM,
     "--classifiers '{gone}/clf.pt': no such file"),
    ("predict-missing+shots0", 1, ["--predict", "{gone}/pics"] + MM + ["DATASET.NUM_SHOTS", "0"],
     "--predict '{gone}/pics': no such directory or list file"),
    ("predict-empty-path+shots0", 1, ["--predict", ""] + MM + ["DATASET.NUM_SHOTS", "0"],
     "--predict: PATH is empty (a directory of images, or a text file with one image path per line)"),
    ("predict-empty-folder+dataset-unknown/zs", 1, ["--predict", "{empty}", "--eval-only", "--trainer", "ZeroshotCLIP", "DATASET.NAME", "Nowhere"],
     "--predict '{empty}': no image file below this directory (" + EXTENSIONS + ")"),
    # --retrieve's pool and --classifiers
    ("retrieve-missing+classifiers/zs", 1, ["--retrieve", "{gone}/pics", "--classifiers", "{clf}"] + ZS,
     "--classifiers '{clf}': --trainer ZeroshotCLIP has no generated classifiers to load (MM_CLS_OP only)"),
    ("retrieve-missing+classifiers-missing", 1, ["--retrieve", "{gone}/pics", "--classifiers", "{gone}/clf.pt"] + MM,
     "--classifiers '{gone}/clf.pt': no such file"),
    ("retrieve-empty-folder+shots0", 1, ["--retrieve", "{empty}"] + MM + ["DATASET.NUM_SHOTS", "0"],
     "--retrieve '{empty}': no image file below this directory (" + EXTENSIONS + ")"),
    ("retrieve-missing+k-transforms", 1, ["--retrieve", "{gone}/pics"] + MM + ["DATALOADER.K_TRANSFORMS", "2"],
     "--retrieve '{gone}/pics': no such directory or list file"),
    # the test pass takes neither --topk nor --classifiers
    ("topk+classifiers+shots0", 1, ["--topk", "3", "--classifiers", "{clf}"] + MM + ["DATASET.NUM_SHOTS", "0"], BELONG_TO_PREDICT),
    ("classifiers+dataset-unknown/zs", 1, ["--classifiers", "{clf}", "--eval-only", "--trainer", "ZeroshotCLIP", "DATASET.NAME", "Nowhere"],
     BELONG_TO_PREDICT),
    ("save-bank+classifiers-missing", 1, ["--save-bank", "--classifiers", "{gone}/clf.pt"] + MM, BELONG_TO_PREDICT),
    # the remaining pairs
    ("retrieve-missing+save-bank+classifiers-missing", 1, ["--retrieve", "{gone}/pics", "--save-bank", "--classifiers", "{gone}/clf.pt"] + MM,
     "--classifiers '{gone}/clf.pt': no such file"),
    ("score-curves0+bank-missing", 1, ["--score-curves", "0", "--bank", "{gone}/bank.pt"] + MM, "--bank '{gone}/bank.pt': no such file"),
    ("score-curves+classifiers+shots0", 1, ["--score-curves", "--classifiers", "{clf}"] + MM + ["DATASET.NUM_SHOTS", "0"], BELONG_TO_PREDICT),
    ("score-curves0+per-class", 1, ["--score-curves", "0", "--per-class", "3"] + MM,
     "--per-class M belongs to --retrieve PATH: the search of an image pool by class"),
    ("nearest0+save-bank+predict-missing", 1, ["--nearest", "0", "--save-bank", "--predict", "{gone}/pics"] + MM,
     "--nearest 0: N must lie in [1, 32]"),
    ("nearest40+topk0+predict", 1, ["--nearest", "40", "--topk", "0", "--predict", "{pics}"] + MM, "--nearest 40: N must lie in [1, 32]"),
    ("nearest+per-class", 1, ["--nearest", "2", "--per-class", "3"] + MM,
     "--per-class M belongs to --retrieve PATH: the search of an image pool by class"),
    ("audit0+topk", 1, ["--audit-bank", "0", "--topk", "3"] + MM, "--audit-bank 0: K must lie in [1, 32]"),
    ("save-bank+per-class/world2", 2, ["--save-bank", "--per-class", "2"] + MM, BANK_ONE_PROCESS),
    ("classifiers+per-class", 1, ["--classifiers", "{clf}", "--per-class", "2"] + MM,
     "--per-class M belongs to --retrieve PATH: the search of an image pool by class"),
    ("bank+remove+per-class", 1, ["--bank", "{bank}", "--remove-classes", "a", "--per-class", "2"] + MM,
     "--per-class M belongs to --retrieve PATH: the search of an image pool by class"),
    # the configuration of a generation
    ("shots0+k-transforms", 1, MM + ["DATASET.NUM_SHOTS", "0", "DATALOADER.K_TRANSFORMS", "2"], SHOTS),
    ("bank+add-missing+shots0", 1, ["--bank", "{bank}", "--add-classes", "{gone}/x"] + MM + ["DATASET.NUM_SHOTS", "0"], SHOTS),
    ("batch-below-shots+k-transforms", 1, MM + ["DATASET.NUM_SHOTS", "4", "DATALOADER.TEST.BATCH_SIZE", "2", "DATALOADER.K_TRANSFORMS", "2"],
     "DATALOADER.TEST.BATCH_SIZE 2 is smaller than DATASET.NUM_SHOTS 4: a loader batch holds whole classes (RandomClassSampler needs one class "
     "per batch), raise TEST.BATCH_SIZE to at least 4"),
    ("k-transforms+audit", 1, ["--audit-bank"] + MM + ["DATASET.NUM_SHOTS", "1", "DATALOADER.K_TRANSFORMS", "2"],
     "DATALOADER.K_TRANSFORMS > 1 only applies to training transforms; the test transform has one view"),
]


@pytest.fixture(scope="module")
def places(tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp("plan")
    (d / "pics").mkdir()
    Image.new("RGB", (8, 8)).save(d / "pics" / "a.png")
    (d / "empty").mkdir()
    for name in ("bank.pt", "clf.pt"):
        (d / name).write_bytes(b"")
    return dict(pics=str(d / "pics"), empty=str(d / "empty"), bank=str(d / "bank.pt"), clf=str(d / "clf.pt"), gone=str(d / "gone"),
                out=str(d / "out"))


def _no_library(monkeypatch):
    from ovmr_amd import checkpoint, runtime

    def boom(*a, **k):
        raise AssertionError("the runner touched the model / library before refusing the job")

    monkeypatch.setattr(runtime, "load_library", boom)
    monkeypatch.setattr(checkpoint, "load_clip_state_dict", boom)


def _argv(arguments, places):
    """The case's arguments on the common command line: weights and a data set that do not exist.  The flags stand first: the KEY VALUE
    opts take the rest of a command line."""
    flags = [a.format(**places) for a in arguments]
    return ["--clip-weights", places["gone"] + "/none.pt", "--root", places["gone"] + "/data", "--output-dir", places["out"]] + flags


def test_table_covers_what_it_promises():
    """Every pair of the runner's job flags stands in at least one case, every case breaks two rules (it names two flags or more), and the
    ids are distinct."""
    import itertools
    flags = ["--predict", "--retrieve", "--score-curves", "--nearest", "--audit-bank", "--bank", "--save-bank", "--classifiers", "--topk",
             "--per-class"]
    edit = {"--add-classes", "--replace-classes", "--remove-classes"}
    used = [{("EDIT" if a in edit else a) for a in c[2] if a.startswith("--")} for c in TABLE]
    missing = [p for p in itertools.combinations(flags + ["EDIT"], 2) if not any(set(p) <= u for u in used)]
    assert not missing, missing
    assert len({c[0] for c in TABLE}) == len(TABLE)
    for zs_flag in ("--bank", "--save-bank", "--nearest", "--audit-bank", "--classifiers", "--score-curves", "EDIT"):
        assert any(zs_flag in u and "ZeroshotCLIP" in c[2] for u, c in zip(used, TABLE)), zs_flag
    for flag in ("--predict", "--bank", "--audit-bank"):
        assert any(flag in u and c[1] == 2 for u, c in zip(used, TABLE)), flag


@pytest.mark.parametrize("world,arguments,message", [c[1:] for c in TABLE], ids=[c[0] for c in TABLE])
def test_main_refuses_with(world, arguments, message, places, monkeypatch):
    from ovmr_amd import cli
    _no_library(monkeypatch)
    monkeypatch.setenv("WORLD_SIZE", str(world))
    with pytest.raises(SystemExit) as e:
        cli.main(_argv(arguments, places))
    assert str(e.value) == message.format(**places)
    assert not os.path.exists(places["out"])


def test_unknown_zero_shot_dataset_is_the_last_refusal_before_the_weights(places, monkeypatch):
    """A data set without a template is refused after the pool was listed, and before torch."""
    from ovmr_amd import cli
    _no_library(monkeypatch)
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(SystemExit, match="Nowhere"):
        cli.main(_argv(["--predict", places["pics"], "--eval-only", "--trainer", "ZeroshotCLIP", "DATASET.NAME", "Nowhere"], places))


# ------------------------------------------------------------------------------------------------ the plan on its own
def _plan(arguments, places):
    from ovmr_amd import cli, config
    args = cli.parse(_argv(arguments, places))
    return cli.plan_job(args, config.setup_cfg(args))


@pytest.mark.parametrize("world,arguments,message", [c[1:] for c in TABLE], ids=[c[0] for c in TABLE])
def test_plan_refuses_as_main(world, arguments, message, places, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", str(world))
    with pytest.raises(SystemExit) as e:
        _plan(arguments, places)
    assert str(e.value) == message.format(**places)


def test_plan_of_every_mode(places, monkeypatch):
    from ovmr_amd import cli
    monkeypatch.setenv("WORLD_SIZE", "1")
    image = [os.path.join(places["pics"], "a.png")]

    p = _plan(MM + ["DATASET.NUM_SHOTS", "2"], places)
    assert (p.mode, p.zeroshot, p.vocabulary, p.edits, p.ragged, p.images, p.lift_shots) == ("test", False, "generate", False, False, [], False)
    assert (p.k, p.m, p.within_top, p.nearest, p.audit, p.curve_bins, p.curve_range, p.skip, p.world) == (None,) * 7 + (False, 1)
    p = _plan(["--ragged-shots", "--save-bank", "--score-curves", "--audit-bank"] + MM + ["DATASET.NUM_SHOTS", "2"], places)
    assert (p.mode, p.vocabulary, p.ragged, p.audit, p.curve_bins, p.curve_range) == ("test", "generate", True, 5, cli.DEFAULT_BINS, (0.0, 1.0))

    p = _plan(["--score-curves", "64", "--score-range", "-5", "40"] + ZS, places)
    assert (p.mode, p.zeroshot, p.vocabulary, p.lift_shots, p.curve_bins, p.curve_range) == ("test", True, "zeroshot", True, 64, (-5.0, 40.0))
    p = _plan(["--ragged-shots", "--predict", places["pics"]] + ZS2, places)
    assert (p.mode, p.k, p.ragged, p.images) == ("predict", 5, False, image)

    p = _plan(["--predict", places["pics"], "--topk", "3", "--nearest", "4"] + MM + ["DATASET.NUM_SHOTS", "2"], places)
    assert (p.mode, p.k, p.nearest, p.vocabulary, p.images, p.lift_shots) == ("predict", 3, 4, "generate", image, False)
    p = _plan(["--ragged-shots", "--predict", places["pics"], "--classifiers", places["clf"]] + MM, places)
    assert (p.mode, p.k, p.vocabulary, p.ragged, p.lift_shots) == ("predict", 5, "classifiers", False, True)

    p = _plan(["--retrieve", places["pics"]] + MM + ["DATASET.NUM_SHOTS", "2"], places)
    assert (p.mode, p.m, p.within_top, p.images) == ("retrieve", cli.MAX_PER_CLASS, None, image)
    monkeypatch.setenv("WORLD_SIZE", "2")
    p = _plan(["--retrieve", places["pics"], "--per-class", "7", "--within-top", "2"] + ZS, places)
    assert (p.mode, p.m, p.within_top, p.world) == ("retrieve", 7, 2, 2)
    monkeypatch.setenv("WORLD_SIZE", "1")

    p = _plan(["--bank", places["bank"], "--audit-bank", "3", "--dup-threshold", "0.9"] + MM, places)
    assert (p.mode, p.vocabulary, p.edits, p.audit, p.lift_shots) == ("audit", "bank", False, 3, True)
    p = _plan(["--bank", places["bank"], "--audit-bank", "--remove-classes", "a"] + MM + ["DATASET.NUM_SHOTS", "2"], places)
    assert (p.mode, p.vocabulary, p.edits, p.audit) == ("test", "bank", True, 5)
    p = _plan(["--bank", places["bank"], "--audit-bank", "--retrieve", places["pics"]] + MM, places)
    assert (p.mode, p.vocabulary, p.audit) == ("retrieve", "bank", 5)


def test_plan_skips_a_job_whose_results_exist(places, tmp_path, monkeypatch, capsys):
    """generate_classifier.sh:27-28: a job that would write mm_classifiers.pt into a folder that holds one is skipped, by the plan's word
    and main's print; a job that writes none (zero-shot, --classifiers, an unedited --bank) runs."""
    from ovmr_amd import cli
    monkeypatch.setenv("WORLD_SIZE", "1")
    (tmp_path / "mm_classifiers.pt").write_bytes(b"")
    here = dict(places, out=str(tmp_path))
    assert _plan(MM + ["DATASET.NUM_SHOTS", "0"], here).skip                  # (the skip comes before the configuration is looked at)
    assert _plan(["--bank", places["bank"], "--remove-classes", "a"] + MM, here).skip
    assert not _plan(["--bank", places["bank"]] + MM, here).skip
    assert not _plan(["--predict", places["pics"], "--classifiers", places["clf"]] + MM, here).skip
    assert not _plan(ZS, here).skip
    _no_library(monkeypatch)
    assert cli.main(_argv(MM, here)) == {}
    assert capsys.readouterr().out == f"Oops! The results exist at {tmp_path} (so skip this job)\n"


def test_planning_imports_no_torch(places):
    """The decode workers re-import ovmr_amd.cli and must stay torch-free; so does everything up to the plan."""
    code = ("import sys\n"
            "from ovmr_amd import cli, config\n"
            f"args = cli.parse({_argv(['--predict', places['pics'], '--topk', '3', '--nearest', '2'] + MM + ['DATASET.NUM_SHOTS', '2'], places)!r})\n"
            "p = cli.plan_job(args, config.setup_cfg(args))\n"
            "assert p.mode == 'predict' and p.k == 3 and len(p.images) == 1, p\n"
            "assert 'torch' not in sys.modules, 'planning a job imported torch'\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, WORLD_SIZE="1"))
    assert r.returncode == 0, r.stderr
