"""Detail mode above the kernel: Classification(per_class=True, confusion=True) on the device against the host evaluator and sklearn, and the
runner's --per-class-result / --confusion-matrix against a --predict --topk 1 run over the same images.  tests/test_hip_eval_detail.py holds
the kernel to the stable descending sort; tests/test_eval_detail_cpu.py holds the host evaluator to the reference's loop.  Run with -m gpu
on an MI355X."""
import csv
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from ovmr_amd import synth

pytestmark = pytest.mark.gpu

SEED = 11


# ----------------------------------------------------------------------------- evaluator
C = 101
CUTS = [0, 256, 512, 549]


def _outputs(kind):
    """549 rows over 101 classes, listed class by class as a test pass lists them.  Class 99 is neither a label nor a prediction, class
    100 is predicted but never a label; about two rows in three carry their largest value on the label, the others elsewhere,
    with ties."""
    g = torch.Generator().manual_seed(7)
    N = CUTS[-1]
    gt = torch.sort(torch.randint(0, 99, (N,), generator=g))[0]
    logits = torch.randint(0, 12, (N, C), generator=g).float()
    logits[:, 99] = -4.0
    logits[3::40, 100] = 13.0                                           # predicted wherever the label is not boosted above it
    boost = torch.rand(N, generator=g) < 0.66
    logits[boost, gt[boost]] = 14.0
    if kind == "probs":
        return torch.softmax(logits, dim=1), gt                         # fp32 probabilities (CustomCLIP.forward)
    return (logits * 1.5).half(), gt                                    # fp16 logits (ZeroshotCLIP.model_inference): exact, ties kept


def _evaluate(device, mo, gt, topk, out):
    from ovmr_amd.evaluator import Classification
    ev = Classification(C, [f"class {i}" for i in range(C)], device=device, per_class=True, confusion=True)
    for a, b in zip(CUTS[:-1], CUTS[1:]):
        ev.process(mo[a:b].to(device), gt[a:b].to(device), **({"topk": topk} if topk != 1 else {}))
    buf = io.StringIO()
    with redirect_stdout(buf):
        res = ev.evaluate(str(out))
    return ev, res, buf.getvalue().replace(str(out), "OUT"), torch.load(out / "cmat.pt", weights_only=False)


@pytest.mark.parametrize("kind,topk", [("probs", 1), ("logits", 1), ("probs", 5)])
def test_device_report_equals_host_and_sklearn(tmp_path, kind, topk):
    from sklearn.metrics import confusion_matrix
    mo, gt = _outputs(kind)
    dev, res_d, text_d, cm_d = _evaluate("cuda", mo, gt, topk, tmp_path / "dev")
    host, res_h, text_h, cm_h = _evaluate("cpu", mo, gt, topk, tmp_path / "host")
    order = torch.sort(mo.float(), dim=1, descending=True, stable=True)[1]
    want = confusion_matrix(gt.numpy(), order[:, 0].numpy(), normalize="true")
    for cm in (cm_d, cm_h):
        assert isinstance(cm, np.ndarray) and cm.dtype == want.dtype and cm.shape == want.shape and np.array_equal(cm, want)
    assert want.shape[0] < C and 100 in order[:, 0].tolist() and 99 not in order[:, 0].tolist()      # reduced to the classes that occur
    assert text_d == text_h and "=> per-class result\n* class: 0 (class 0)\ttotal: " in text_d     # the whole output, per-class block included
    assert list(res_d) == ["accuracy", "error_rate", "macro_f1", "perclass_accuracy"] and dict(res_d) == dict(res_h)
    # perclass_accuracy from the definition: the mean over the classes with a label of 100 * (top-k) matches / total
    hit = (order[:, :topk] == gt.unsqueeze(1)).any(dim=1)
    accs = [100.0 * int(hit[gt == c].sum()) / int((gt == c).sum()) for c in range(C) if bool((gt == c).any())]
    assert res_d["perclass_accuracy"] == float(np.mean(accs)) and res_d["accuracy"] == pytest.approx(100.0 * float(hit.float().mean()))
    assert torch.equal(dev.confusion_counts, host.confusion_counts) and dev.confusion_counts.dtype == torch.int64
    assert int(dev.confusion_counts.sum()) == CUTS[-1]
    for name in ("acc_per_class.csv", "f1_per_class.csv"):
        assert (tmp_path / "dev" / name).read_bytes() == (tmp_path / "host" / name).read_bytes()


def test_device_detail_pass_makes_one_launch_per_batch(monkeypatch):
    """Detail mode goes through ovmr_eval_detail alone: neither of the two launches it replaces is made."""
    from ovmr_amd import runtime
    from ovmr_amd.evaluator import Classification
    mo, gt = _outputs("logits")
    calls = []
    real = runtime.eval_detail
    monkeypatch.setattr(runtime, "eval_detail", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(runtime, "topk_rows", lambda *a, **k: pytest.fail("ovmr_topk_rows launched in detail mode"))
    ev = Classification(C, device="cuda", per_class=True)
    for a, b in zip(CUTS[:-1], CUTS[1:]):
        ev.process(mo[a:b].cuda(), gt[a:b].cuda(), topk=5)
    assert len(calls) == 3 and ev._cmat is None and ev._class_hits is not None


# ----------------------------------------------------------------------------- runner
NAMES = ["accordion", "sea_horse", "stop_sign", "yin_yang"]
PER_CLASS = [2, 2, 2, 1]                                               # seven test images over four classes


def _pl_state(name="tiny", n_ctx=2):
    return {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(synth.SPECS[name], n_ctx, SEED, True).items()}


def _dataset(tmp_path, golden, spec):
    """Class folders with two PNG exemplars each (train) and seven JPEG test images (val), the BPE fixture, the CLIP weights."""
    from PIL import Image
    from test_zeroshot_cpu import zsclip_bpe
    rng = np.random.default_rng(3)
    root = tmp_path / "data"
    i = 0
    for c in range(len(NAMES)):
        d = root / "train" / f"n{c:02d}"
        d.mkdir(parents=True)
        for j in range(2):
            base = np.full((70, 90, 3), 40 * c + 30, dtype=np.int32) + rng.integers(-25, 25, (70, 90, 3))
            Image.fromarray(base.clip(0, 255).astype(np.uint8)).save(d / f"{j}.png")
        d = root / "val" / f"n{c:02d}"
        d.mkdir(parents=True)
        for j in range(PER_CLASS[c]):
            base = np.full((50 + 3 * i, 80 - 2 * i, 3), 35 * i + 20, dtype=np.int32) + rng.integers(-20, 20, (50 + 3 * i, 80 - 2 * i, 3))
            Image.fromarray(base.clip(0, 255).astype(np.uint8)).save(d / f"img{i}.jpg", quality=92)
            i += 1
    (root / "classnames.txt").write_text("".join(f"n{c:02d} {n}\n" for c, n in enumerate(NAMES)))
    bpe = str(tmp_path / "bpe.txt.gz")
    zsclip_bpe(bpe, golden)
    clip_sd = {k: torch.from_numpy(v) for k, v in synth.clip_state_dict(spec, SEED, jitter=True).items()}
    torch.save(clip_sd, tmp_path / "clip.pt")
    return root, bpe


def _want_block(y_true, y_pred):
    lines = ["=> per-class result"]
    accs = []
    for c in sorted(set(y_true)):
        total = sum(1 for t in y_true if t == c)
        correct = sum(1 for t, p in zip(y_true, y_pred) if t == c and p == c)
        accs.append(100.0 * correct / total)
        lines.append(f"* class: {c} ({NAMES[c]})\ttotal: {total:,}\tcorrect: {correct:,}\tacc: {accs[-1]:.1f}%")
    lines.append(f"* average: {np.mean(accs):.1f}%")
    return "\n".join(lines) + "\n", float(np.mean(accs))


@pytest.mark.parametrize("trainer", ["ZeroshotCLIP", "MM_CLS_OP"])
def test_runner_flags(golden, tmp_path, capsys, trainer):
    from sklearn.metrics import confusion_matrix
    from ovmr_amd import checkpoint, cli
    spec, B = synth.SPECS["tiny"], 3
    R = spec.image_resolution
    root, bpe = _dataset(tmp_path, golden, spec)
    argv = ["--root", str(root), "--seed", "1", "--trainer", trainer, "--eval-only", "--clip-weights", str(tmp_path / "clip.pt"),
            "--bpe-path", bpe, "--workers", "2"]
    if trainer == "MM_CLS_OP":
        checkpoint.save_prompt_learner_state(_pl_state(), str(tmp_path / "ckpt"), 30)
        argv += ["--model-dir", str(tmp_path / "ckpt"), "--load-epoch", "30", "--eval_mode", "fusion", "--eval_tau", "10", "--n_ctx", "2"]
        opts = ["DATASET.NAME", "ImageNet", "INPUT.SIZE", f"({R}, {R})", "DATALOADER.TEST.BATCH_SIZE", "4", "DATASET.NUM_SHOTS", "2"]
        model_files = ["mm_classifiers.pt", "visual_tokens.pt"]
    else:
        opts = ["DATASET.NAME", "Caltech101", "INPUT.SIZE", f"({R}, {R})", "DATALOADER.TEST.BATCH_SIZE", str(B)]
        model_files = []
    items = cli.list_split(str(root), "val")[1]
    y_true = [label for _, label in items]
    assert y_true == [0, 0, 1, 1, 2, 2, 3]

    out = tmp_path / "out"
    capsys.readouterr()
    res = cli.main(argv + ["--output-dir", str(out), "--per-class-result", "--confusion-matrix"] + opts)
    text = capsys.readouterr().out
    assert sorted(p.name for p in out.iterdir()) == sorted(["acc_per_class.csv", "cmat.pt", "f1_per_class.csv"] + model_files)

    # the rank-0 class of a prediction pass over the same images, in the same order
    lst = tmp_path / "val.txt"
    lst.write_text("".join(f"{p}\n" for p, _ in items))
    extra = ["--classifiers", str(out / "mm_classifiers.pt")] if trainer == "MM_CLS_OP" else []
    pred = cli.main(argv + ["--output-dir", str(tmp_path / "pred"), "--predict", str(lst), "--topk", "1"] + extra + opts)
    y_pred = [ranks[0][0] for _, ranks in pred["predictions"]]
    assert [p for p, _ in pred["predictions"]] == [p for p, _ in items]

    want = confusion_matrix(y_true, y_pred, normalize="true")
    got = torch.load(out / "cmat.pt", weights_only=False)
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
    block, mean = _want_block(y_true, y_pred)
    assert block in text and f"Confusion matrix is saved to {out / 'cmat.pt'}\n" in text
    assert res["perclass_accuracy"] == mean
    assert res["accuracy"] == pytest.approx(100.0 * sum(t == p for t, p in zip(y_true, y_pred)) / len(y_true))
    # acc_per_class.csv against the matrix's diagonal (every class has a label here, so matrix row i is class i)
    rows = list(csv.reader((out / "acc_per_class.csv").read_text().splitlines()))
    assert rows[0] == ["Label", "Acc"] and [r[0] for r in rows[1:]] == ["0", "1", "2", "3"]
    present = sorted(set(y_true) | set(y_pred))
    for label, acc in rows[1:]:
        i = present.index(int(label))
        assert float(acc) == pytest.approx(100.0 * got[i, i], abs=1e-9)      # two float64 roundings apart at the most

    # the same command without the flags: today's files, today's keys, no per-class block
    plain = tmp_path / "plain"
    capsys.readouterr()
    res0 = cli.main(argv + ["--output-dir", str(plain)] + opts)
    text0 = capsys.readouterr().out
    assert sorted(p.name for p in plain.iterdir()) == sorted(["acc_per_class.csv", "f1_per_class.csv"] + model_files)
    assert "perclass_accuracy" not in res0 and "per-class result" not in text0 and "Confusion matrix" not in text0
    assert all(res0[key] == res[key] for key in ("accuracy", "error_rate", "macro_f1"))
    for name in ("acc_per_class.csv", "f1_per_class.csv"):
        assert (plain / name).read_bytes() == (out / name).read_bytes()
