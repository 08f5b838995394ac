"""Host side of ranked prediction: Classification.process(mo, gt, topk) on host tensors against the reference's literal formula
(Dassl.pytorch/dassl/evaluation/evaluator.py:56-60), the TEST.TOPK key, the runner's --predict refusals and the predictions.csv writer.
No GPU."""
import numpy as np
import pytest
import torch

NAN, INF = float("nan"), float("inf")


def _reference_correct(pred, gt, topk):
    """evaluator.py:58-59 on the given [B, topk] predictions."""
    matches = (pred == (gt.unsqueeze(1).repeat(1, topk))).float().sum(dim=-1)
    return int(matches.sum().item())


def _stable(mo, k):
    return torch.sort(mo.float(), dim=1, descending=True, stable=True)[1][:, :k]


def _run(mo, gt, k, cuts, tmp_path=None):
    from ovmr_amd.evaluator import Classification
    ev = Classification(mo.shape[1], device="cpu")
    for a, b in zip(cuts[:-1], cuts[1:]):
        ev.process(mo[a:b], gt[a:b], topk=k)
    return ev, ev.evaluate(str(tmp_path) if tmp_path else None)


@pytest.mark.parametrize("k", [2, 5])
def test_host_topk_equals_the_reference_formula_without_ties(k, capsys):
    B, C = 50, 23
    rng = np.random.default_rng(k)
    mo = torch.from_numpy(np.stack([rng.permutation(C) for _ in range(B)]).astype(np.float32))      # no tie in any row
    gt = torch.from_numpy(rng.integers(0, C, B))
    _, res = _run(mo, gt, k, [0, 17, 17, 40, B])
    correct = _reference_correct(mo.topk(k=k, dim=-1)[1], gt, k)                                     # :57, valid without ties
    assert 0 < correct < B
    assert res["accuracy"] == pytest.approx(100.0 * correct / B) and res["error_rate"] == pytest.approx(100.0 - res["accuracy"])
    out = capsys.readouterr().out
    assert f"* total: {B:,}\n* correct: {correct:,}\n* accuracy: {100.0 * correct / B:.1f}%\n" in out


def test_host_topk_with_ties_uses_the_stable_order(tmp_path):
    B, C, k = 40, 12, 3
    g = torch.Generator().manual_seed(0)
    mo = torch.randint(0, 4, (B, C), generator=g).float()                # four values over twelve columns: ties in every row
    mo[0, :10] = torch.tensor([1, NAN, 3, 3, -0.0, 0.0, INF, NAN, -INF, 3])
    mo[1] = 2.0
    gt = torch.randint(0, C, (B,), generator=g)
    gt[0], gt[1] = 6, 3                                                   # rank 2 of row 0 (NaN, NaN, inf): a hit; column 3 of a constant row: a miss
    ev, res = _run(mo, gt, k, [0, 13, 27, B], tmp_path / "k3")
    order = _stable(mo, k)
    assert order[0].tolist() == [1, 7, 6] and order[1].tolist() == [0, 1, 2]
    correct = _reference_correct(order, gt, k)
    assert res["accuracy"] == pytest.approx(100.0 * correct / B)
    # macro-F1 and both CSVs come from the top-1 prediction (:64-65): byte-equal to a topk = 1 pass, whose accuracy is the top-1 accuracy
    ev1, res1 = _run(mo, gt, 1, [0, 13, 27, B], tmp_path / "k1")
    assert res1["macro_f1"] == res["macro_f1"] and res1["accuracy"] == pytest.approx(100.0 * float((order[:, 0] == gt).float().mean()))
    assert res1["accuracy"] < res["accuracy"]
    for name in ("acc_per_class.csv", "f1_per_class.csv"):
        assert (tmp_path / "k3" / name).read_bytes() == (tmp_path / "k1" / name).read_bytes()
    assert all(torch.equal(a, b) for a, b in zip(ev.counts(), ev1.counts()))


def test_one_pass_uses_one_topk():
    from ovmr_amd.evaluator import Classification
    ev = Classification(6, device="cpu")
    mo, gt = torch.rand(4, 6), torch.tensor([0, 1, 2, 3])
    ev.process(mo, gt, topk=3)
    with pytest.raises(ValueError, match="one topk"):
        ev.process(mo, gt)
    with pytest.raises(ValueError, match="one topk"):
        ev.process(mo, gt, topk=2)
    ev.reset()
    ev.process(mo, gt)                                                    # the default is top-1, today's path
    with pytest.raises(ValueError, match="one topk"):
        ev.process(mo, gt, topk=3)
    ev.reset()
    for bad in (0, 7, 33):
        with pytest.raises(ValueError, match="topk"):
            ev.process(mo, gt, topk=bad)
    # a label outside [0, C) never hits (and is still reported by counts())
    ev.process(mo, torch.tensor([0, 1, -1, 6]), topk=6)
    assert int(ev._hits) == 2


def test_test_topk_key():
    from types import SimpleNamespace
    from ovmr_amd import config
    assert config.DEFAULTS["TEST.TOPK"] == 1
    assert config.setup_cfg(SimpleNamespace(opts=[])).TEST.TOPK == 1
    assert config.setup_cfg(SimpleNamespace(opts=["TEST.TOPK", "5"])).TEST.TOPK == 5
    with pytest.raises(ValueError):
        config.setup_cfg(SimpleNamespace(opts=["TEST.TOPK", "five"]))
    cfg = config.setup_cfg(SimpleNamespace(opts=["TEST.PER_CLASS_RESULT", "True", "TEST.COMPUTE_CMAT", "True"]))    # still accepted, still ignored
    assert not hasattr(cfg.TEST, "PER_CLASS_RESULT") and not hasattr(cfg.TEST, "COMPUTE_CMAT")


def test_trainer_passes_test_topk():
    """_EvalTrainer.test() on the host: TEST.TOPK reaches process(); without the key the pass is top-1."""
    from types import SimpleNamespace
    from ovmr_amd import trainer
    C = 4
    mo = torch.tensor([[.1, .2, .3, .4], [.4, .3, .2, .1], [.1, .4, .3, .2], [.3, .1, .2, .4]])
    gt = torch.tensor([2, 1, 0, 1])                                      # ranks 1, 1, 3, 3

    class Host(trainer._EvalTrainer):
        def build_model(self):
            pass

        def parse_batch_test(self, batch):
            return batch["img"], batch["label"]

        def outputs(self, inputs):
            for x in inputs:
                yield x

    def run(test_ns):
        cfg = SimpleNamespace(OUTPUT_DIR="", **test_ns)
        dm = SimpleNamespace(dataset=SimpleNamespace(classnames=list("abcd")), test_loader=[{"img": mo[:3], "label": gt[:3]}, {"img": mo[3:], "label": gt[3:]}])
        return Host(cfg, dm, device="cpu").test()

    assert run({}) == pytest.approx(0.0)
    assert run({"TEST": SimpleNamespace(TOPK=1, SPLIT="test")}) == pytest.approx(0.0)
    assert run({"TEST": SimpleNamespace(TOPK=2, SPLIT="test")}) == pytest.approx(50.0)
    assert run({"TEST": SimpleNamespace(TOPK=4, SPLIT="test")}) == pytest.approx(100.0)


def _no_library(monkeypatch):
    from ovmr_amd import checkpoint, runtime

    def boom(*a, **k):
        raise AssertionError("the runner touched the model / library before refusing the job")

    monkeypatch.setattr(runtime, "load_library", boom)
    monkeypatch.setattr(checkpoint, "load_clip_state_dict", boom)


@pytest.mark.parametrize("trainer", ["MM_CLS_OP", "ZeroshotCLIP"])
def test_predict_refusals_come_before_anything_is_loaded(monkeypatch, tmp_path, trainer):
    from PIL import Image
    from ovmr_amd import cli
    _no_library(monkeypatch)
    monkeypatch.setenv("WORLD_SIZE", "1")
    pics = tmp_path / "pics"
    (pics / "sub").mkdir(parents=True)
    Image.new("RGB", (8, 8)).save(pics / "sub" / "a.png")
    (pics / "notes.txt").write_text("not an image")
    empty = tmp_path / "empty"
    empty.mkdir()
    (empty / "readme.txt").write_text("no image here")
    base = ["--root", str(tmp_path / "nowhere"), "--trainer", trainer, "--eval-only", "--clip-weights", str(tmp_path / "none.pt"),
            "--output-dir", str(tmp_path / "out"), "DATASET.NAME", "Caltech101", "DATASET.NUM_SHOTS", "1"]
    pred = ["--predict", str(pics)]
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="--predict runs in one process"):
        cli.main(pred + base)
    monkeypatch.setenv("WORLD_SIZE", "1")
    for bad in ("0", "33", "-1"):
        with pytest.raises(SystemExit, match=f"--topk {bad}"):
            cli.main(pred + ["--topk", bad] + base)
    with pytest.raises(SystemExit, match="empty.*no image file"):
        cli.main(["--predict", str(empty)] + base)
    with pytest.raises(SystemExit, match="--predict: PATH is empty"):
        cli.main(["--predict", ""] + base)
    with pytest.raises(SystemExit, match="missing.txt"):
        cli.main(["--predict", str(tmp_path / "missing.txt")] + base)
    lst = tmp_path / "list.txt"
    lst.write_text(f"{pics / 'sub' / 'a.png'}\n\n{tmp_path / 'gone.jpg'}\n")
    with pytest.raises(SystemExit, match=r"list.txt:3: .*gone.jpg"):
        cli.main(["--predict", str(lst)] + base)
    (tmp_path / "blank.txt").write_text("\n\n")
    with pytest.raises(SystemExit, match="blank.txt.*names no image"):
        cli.main(["--predict", str(tmp_path / "blank.txt")] + base)
    with pytest.raises(SystemExit, match="--predict"):
        cli.main(["--topk", "3"] + base)                                  # --topk without --predict
    clf = tmp_path / "mm_classifiers.pt"
    clf.write_bytes(b"")
    if trainer == "ZeroshotCLIP":
        with pytest.raises(SystemExit, match="--classifiers.*ZeroshotCLIP"):
            cli.main(pred + ["--classifiers", str(clf)] + base)
    else:
        with pytest.raises(SystemExit, match="--classifiers.*nothing.pt"):
            cli.main(pred + ["--classifiers", str(tmp_path / "nothing.pt")] + base)
    assert not (tmp_path / "out").exists()


def test_topk_larger_than_the_class_list_is_refused_before_the_weights(monkeypatch, tmp_path):
    from PIL import Image
    from ovmr_amd import cli
    _no_library(monkeypatch)
    monkeypatch.setenv("WORLD_SIZE", "1")
    for split in ("train", "val"):
        for c in range(3):
            d = tmp_path / "data" / split / f"n{c}"
            d.mkdir(parents=True)
            Image.new("RGB", (8, 8)).save(d / "0.png")
    with pytest.raises(SystemExit, match=r"--topk 4: .*3 classes"):
        cli.main(["--predict", str(tmp_path / "data" / "val"), "--topk", "4", "--root", str(tmp_path / "data"), "--trainer", "ZeroshotCLIP",
                  "--eval-only", "--clip-weights", str(tmp_path / "none.pt"), "--output-dir", str(tmp_path / "out"), "DATASET.NAME", "Caltech101"])
    assert not (tmp_path / "out").exists()


def test_list_predict_images_orders(tmp_path):
    from ovmr_amd import cli
    for name in ("b/2.jpg", "b/10.JPG", "a/z.png", ".hidden/x.png", "a/.skip.png", "c.jpeg", "a/notes.txt"):
        p = tmp_path / "pics" / name
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"x")
    root = str(tmp_path / "pics")
    got = cli.list_predict_images(root)
    assert got == sorted(got) and [p[len(root) + 1:] for p in got] == ["a/z.png", "b/10.JPG", "b/2.jpg", "c.jpeg"]
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join([got[2], got[0], got[2]]) + "\n")
    assert cli.list_predict_images(str(lst)) == [got[2], got[0], got[2]]                  # file order, repeats kept


def test_predictions_csv_writer(tmp_path):
    import csv
    from ovmr_amd import cli
    names = ["sea horse", "stop, sign", "yin_yang"]
    values = torch.tensor([[0.7, 0.1 + 0.2], [NAN, INF]], dtype=torch.float32)
    indices = torch.tensor([[2, 0], [1, 2]])
    preds = cli.ranked_predictions(["im/a.jpg", "im/b, c.jpg"], values, indices, names)
    assert preds[0] == ("im/a.jpg", [(2, "yin_yang", float(values[0, 0])), (0, "sea horse", float(values[0, 1]))])
    path = tmp_path / "deep" / "predictions.csv"
    cli.write_predictions(str(path), preds)
    text = path.read_text()
    lines = text.split("\n")
    assert lines[0] == "image,rank,label,classname,score" and lines[-1] == "" and len(lines) == 1 + 4 + 1
    assert lines[1] == f"im/a.jpg,0,2,yin_yang,{float(values[0, 0])!r}"
    rows = list(csv.reader(text.splitlines()))[1:]
    assert [r[0] for r in rows] == ["im/a.jpg", "im/a.jpg", "im/b, c.jpg", "im/b, c.jpg"] and [r[1] for r in rows] == ["0", "1", "0", "1"]
    assert [r[3] for r in rows] == ["yin_yang", "sea horse", "stop, sign", "yin_yang"]
    back = torch.tensor([float(r[4]) for r in rows], dtype=torch.float32).reshape(2, 2)
    assert torch.equal(torch.isnan(back), torch.isnan(values)) and torch.equal(back[0], values[0]) and back[1, 1] == INF
