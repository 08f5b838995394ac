"""Detail mode of the evaluator on host tensors (ovmr_amd/evaluator.py: per_class= / confusion=): cmat.pt against
sklearn.metrics.confusion_matrix(normalize="true"), the `=> per-class result` block against a literal restatement of the reference's loop
(Dassl.pytorch/dassl/evaluation/evaluator.py:50-73, 140-163), the unchanged default path, and the runner's refusal of the two flags together
with --predict.  The comparators of this file are themselves shown to reject the defects they are there to catch."""
import io
from collections import defaultdict
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

C = 7
NAMES = [f"name {i}" for i in range(C)]
CUTS = [0, 9, 10, 23]                                                  # three batches; the second holds one image


def _job():
    """23 rows over 7 classes: class 5 is neither a label nor a prediction, class 6 is predicted but never a label; ties in some rows."""
    g = torch.Generator().manual_seed(3)
    mo = torch.randint(0, 5, (CUTS[-1], C), generator=g).float()
    mo[:, 5] = -3.0                                                     # never among the best
    gt = torch.randint(0, 5, (CUTS[-1],), generator=g)
    mo[4, 6] = mo[11, 6] = 9.0                                          # class 6: predicted, never labelled
    mo[2] = 1.0                                                         # an all-equal row: column 0
    return mo, gt


def _reference(mo, gt, topk, names):
    """evaluator.py:50-73 and :140-163 restated: returns (printed block, perclass_accuracy, y_true, y_pred).  The ranking is the stable
    descending sort (the library's total order), where the reference calls mo.topk."""
    per_class_res, y_true, y_pred = defaultdict(list), [], []
    for a, b in zip(CUTS[:-1], CUTS[1:]):
        m, g = mo[a:b], gt[a:b]
        pred = torch.sort(m, dim=1, descending=True, stable=True)[1][:, :topk]
        matches = (pred == (g.unsqueeze(1).repeat(1, topk))).float().sum(dim=-1)
        y_true.extend(g.numpy().tolist())
        y_pred.extend(pred[:, 0].numpy().tolist())
        for i, label in enumerate(g):
            per_class_res[label.item()].append(int(matches[i].item()))
    labels = sorted(per_class_res.keys())
    lines, accs = ["=> per-class result"], []
    for label in labels:
        res = per_class_res[label]
        correct, total = sum(res), len(res)
        acc = 100.0 * correct / total
        accs.append(acc)
        lines.append(f"* class: {label} ({names[label]})\t" f"total: {total:,}\t" f"correct: {correct:,}\t" f"acc: {acc:.1f}%")
    mean_acc = np.mean(accs)
    lines.append(f"* average: {mean_acc:.1f}%")
    return "\n".join(lines) + "\n", mean_acc, y_true, y_pred


def _run(mo, gt, topk=1, out=None, **kw):
    from ovmr_amd.evaluator import Classification
    ev = Classification(C, NAMES, device="cpu", **kw)
    for a, b in zip(CUTS[:-1], CUTS[1:]):
        ev.process(mo[a:b], gt[a:b], **({"topk": topk} if topk != 1 else {}))
    buf = io.StringIO()
    with redirect_stdout(buf):
        res = ev.evaluate(str(out) if out else None)
    return ev, res, buf.getvalue()


def _block(text):
    """The per-class block of evaluate()'s output: from its headline to the average line."""
    a = text.index("=> per-class result")
    b = text.index("\n", text.index("* average:", a)) + 1
    return text[a:b]


def same_matrix(got, want):
    return isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("topk", [1, 3])
def test_cmat_and_per_class_block_equal_sklearn_and_the_reference(tmp_path, topk):
    from sklearn.metrics import confusion_matrix, f1_score
    mo, gt = _job()
    want_block, want_mean, y_true, y_pred = _reference(mo, gt, topk, NAMES)
    assert 5 not in y_true + y_pred and 6 in y_pred and 6 not in y_true
    ev, res, text = _run(mo, gt, topk, tmp_path, per_class=True, confusion=True)
    want = confusion_matrix(y_true, y_pred, normalize="true")
    got = torch.load(tmp_path / "cmat.pt", weights_only=False)
    assert want.shape == (6, 6) and want.dtype == np.float64
    assert same_matrix(got, want)
    assert f"Confusion matrix is saved to {tmp_path / 'cmat.pt'}\n" in text
    assert _block(text) == want_block
    assert text.index("=> result") < text.index("=> per-class result") < text.index("Confusion matrix is saved")
    assert list(res) == ["accuracy", "error_rate", "macro_f1", "perclass_accuracy"]
    assert isinstance(res["perclass_accuracy"], float) and res["perclass_accuracy"] == float(want_mean)
    raw = ev.confusion_counts
    assert raw.dtype == torch.int64 and raw.shape == (C, C)
    assert np.array_equal(raw.numpy(), confusion_matrix(y_true, y_pred, labels=list(range(C))))
    # the confusion matrix and F1 stay top-1 whatever topk is
    assert res["macro_f1"] == pytest.approx(100.0 * f1_score(y_true, y_pred, average="macro", labels=np.unique(y_true)))
    if topk == 3:
        ev1, res1, text1 = _run(mo, gt, 1, tmp_path / "k1", per_class=True, confusion=True)
        assert torch.equal(ev1.confusion_counts, raw) and res1["macro_f1"] == res["macro_f1"]
        assert _block(text1) != want_block and res1["perclass_accuracy"] < res["perclass_accuracy"]      # top-k matches, not top-1
        assert same_matrix(torch.load(tmp_path / "k1" / "cmat.pt", weights_only=False), want)


def test_each_option_alone(tmp_path):
    mo, gt = _job()
    ev, res, text = _run(mo, gt, 3, tmp_path / "a", per_class=True)
    assert "perclass_accuracy" in res and "=> per-class result" in text and ev.confusion_counts is None
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["acc_per_class.csv", "f1_per_class.csv"]
    ev, res, text = _run(mo, gt, 3, tmp_path / "b", confusion=True)
    assert list(res) == ["accuracy", "error_rate", "macro_f1"] and "per-class" not in text
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == ["acc_per_class.csv", "cmat.pt", "f1_per_class.csv"]
    ev, res, text = _run(mo, gt, 1, None, confusion=True)               # no output_dir: the raw counts only
    assert int(ev.confusion_counts.sum()) == CUTS[-1] and "Confusion matrix" not in text
    ev.reset()
    assert ev.confusion_counts is None and ev._cmat is None


def test_default_evaluator_is_unchanged(tmp_path):
    mo, gt = _job()
    ev, res, text = _run(mo, gt, 1, tmp_path)
    assert list(res) == ["accuracy", "error_rate", "macro_f1"]
    assert "per-class" not in text and "Confusion" not in text and text.startswith("=> result\n") and text.count("\n") == 6
    assert sorted(p.name for p in tmp_path.iterdir()) == ["acc_per_class.csv", "f1_per_class.csv"]
    assert ev._cmat is None and ev._class_hits is None and ev.confusion_counts is None
    ev3, res3, text3 = _run(mo, gt, 3, tmp_path / "k3")
    assert list(res3) == ["accuracy", "error_rate", "macro_f1"] and text3.count("\n") == 6


def test_out_of_range_label_raises():
    mo, gt = _job()
    for bad in (-1, C):
        g2 = gt.clone()
        g2[7] = bad
        from ovmr_amd.evaluator import Classification
        ev = Classification(C, NAMES, device="cpu", per_class=True, confusion=True)
        ev.process(mo, g2, topk=3)
        assert int(ev._cmat.sum()) == CUTS[-1] - 1 and int(ev._counts[2 * C:3 * C].sum()) == CUTS[-1] - 1      # the row is counted nowhere else
        with pytest.raises(ValueError, match="outside"):
            ev.evaluate()


@pytest.mark.parametrize("trainer", ["MM_CLS_OP", "ZeroshotCLIP", "ZeroshotCLIP2"])
@pytest.mark.parametrize("flag", ["--per-class-result", "--confusion-matrix"])
def test_runner_refuses_the_flags_with_predict_before_anything_is_loaded(monkeypatch, tmp_path, trainer, flag):
    from PIL import Image
    from ovmr_amd import checkpoint, cli, runtime

    def boom(*a, **k):
        raise AssertionError("the runner touched the model / library before refusing the job")

    monkeypatch.setattr(runtime, "load_library", boom)
    monkeypatch.setattr(checkpoint, "load_clip_state_dict", boom)
    monkeypatch.setenv("WORLD_SIZE", "1")
    pics = tmp_path / "pics"
    pics.mkdir()
    Image.new("RGB", (8, 8)).save(pics / "a.png")
    base = ["--root", str(tmp_path / "nowhere"), "--trainer", trainer, "--eval-only", "--clip-weights", str(tmp_path / "none.pt"),
            "--output-dir", str(tmp_path / "out"), "DATASET.NAME", "Caltech101", "DATASET.NUM_SHOTS", "1"]
    with pytest.raises(SystemExit, match=flag):
        cli.main(["--predict", str(pics), flag] + base)
    assert not (tmp_path / "out").exists()
    args = cli.parse([flag] + base)                                     # without --predict the flag parses, the other stays off
    assert args.per_class_result == (flag == "--per-class-result") and args.confusion_matrix == (flag == "--confusion-matrix")


def test_trainers_hand_the_options_to_their_evaluator():
    import inspect
    from ovmr_amd import trainer
    for cls in (trainer.MM_CLS_OP, trainer.ZeroshotCLIP, trainer.ZeroshotCLIP2):
        p = inspect.signature(cls.__init__).parameters
        assert p["per_class_result"].default is False and p["compute_cmat"].default is False


# ----------------------------------------------------------------------------- the comparators reject what they are there to catch
def test_the_comparators_reject_the_known_defects():
    from sklearn.metrics import confusion_matrix
    mo, gt = _job()
    want_block, _, y_true, y_pred = _reference(mo, gt, 1, NAMES)
    want = confusion_matrix(y_true, y_pred, normalize="true")
    assert same_matrix(want.copy(), want)
    assert not same_matrix(want.T.copy(), want)                                                  # transposed
    full = confusion_matrix(y_true, y_pred, labels=list(range(C)), normalize="true")
    assert not same_matrix(full, want)                                                           # unreduced [C, C]
    assert not same_matrix(confusion_matrix(y_true, y_pred, normalize="pred"), want)             # column-normalised
    assert not same_matrix(want.astype(np.float32), want)                                        # another dtype
    assert not same_matrix(torch.from_numpy(want), want)                                         # not the NumPy array
    lines = want_block.splitlines(keepends=True)
    absent = f"* class: 5 ({NAMES[5]})\ttotal: 0\tcorrect: 0\tacc: 0.0%\n"
    listed = "".join(lines[:-1]) + absent + lines[-1]                                            # a block that lists an absent class
    text = "=> result\n* total: 23\n" + listed + "trailer\n"
    assert _block("=> result\n" + want_block + "trailer\n") == want_block
    assert _block(text) == listed != want_block
