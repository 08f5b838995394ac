"""Score curves through the evaluator and the runner (`pytest -m gpu`): Classification(curves=...) on the device against the host
evaluator on the same outputs, then the synthetic-folder job of tests/test_hip_eval_report.py with `--score-curves` -- in one process,
and as 2 and 3 ranks sharing the GPU over gloo (tests/eval_shard_worker.py; seven test images in batches of 4: a count the world sizes
do not divide, and at world 3 a rank without an image) -- whose curve files must be byte-equal across the three runs and whose other
files and result lines must be those of the same job without the flag.  Exact."""
import csv
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import curves_cases as K
from ovmr_amd import synth

pytestmark = pytest.mark.gpu
CURVE_FILES = ["curves_per_class.csv", "score_hist.pt"]


@pytest.mark.parametrize("kind,bins,score_range", [("probs", 256, (0.0, 1.0)), ("logits", 4096, (-8.0, 22.0)), ("probs", 7, (0.1, 0.7))])
def test_device_evaluator_equals_host(tmp_path, kind, bins, score_range, monkeypatch):
    from ovmr_amd import runtime
    from ovmr_amd.evaluator import Classification
    from test_hip_eval_report import C, CUTS, _outputs
    mo, gt = _outputs(kind)
    edges = torch.from_numpy(K.edge_table(*score_range, bins, fp16=mo.dtype == torch.float16)).to(mo.dtype)
    mo.view(-1)[torch.randperm(mo.numel(), generator=torch.Generator().manual_seed(1))[:len(edges)]] = edges
    launches = []
    real = runtime.eval_curves
    monkeypatch.setattr(runtime, "eval_curves", lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    got = {}
    for device in ("cuda", "cpu"):
        ev = Classification(C, [f"class {i}" for i in range(C)], device=device, per_class=device == "cuda", curves=bins, score_range=score_range)
        for a, b in zip(CUTS[:-1], CUTS[1:]):
            ev.process(mo[a:b].to(device), gt[a:b].to(device))
        buf = io.StringIO()
        with redirect_stdout(buf):
            res = ev.evaluate(str(tmp_path / device))
        got[device] = (ev, res, [l for l in buf.getvalue().splitlines() if l.startswith(("* mAP", "* mean_auroc"))])
    assert len(launches) == 3, "one launch per batch, on the device only"
    dev, host = got["cuda"][0], got["cpu"][0]
    assert dev._curves.is_cuda and dev._curves.dtype == torch.int32 and torch.equal(dev._curves.cpu(), host._curves)
    assert K.mismatch(dev._curves.cpu(), K.expected(mo, gt, *score_range, bins)) is None
    assert torch.equal(dev.score_hist, host.score_hist) and int(dev.score_hist.sum()) == CUTS[-1] * C
    assert got["cuda"][1]["mAP"] == got["cpu"][1]["mAP"] and got["cuda"][1]["mean_auroc"] == got["cpu"][1]["mean_auroc"]
    assert got["cuda"][2] == got["cpu"][2] and len(got["cuda"][2]) == 2
    for k in dev.curves:
        assert np.array_equal(dev.curves[k], host.curves[k], equal_nan=True), k
    for name in CURVE_FILES:
        assert (tmp_path / "cuda" / name).read_bytes() == (tmp_path / "cpu" / name).read_bytes(), name
    rows = list(csv.reader(open(tmp_path / "cuda" / "curves_per_class.csv")))
    assert len(rows) == 1 + C and rows[100][2:] == ["0", str(CUTS[-1])] + [""] * 7, "class 99 is never a label"


def _lines(text, out):
    from test_hip_eval_shard import _blocks
    return _blocks(text, out)


def _curve_lines(lines):
    return [l for l in lines if l.startswith(("* mAP: ", "* mean_auroc: "))]


@pytest.mark.timeout(900)
def test_runner_all_modes_one_two_and_three_ranks(golden, tmp_path):
    from test_hip_eval_shard import _job, _job_result, _mm_cls_op_argv, _tree
    from ovmr_amd.runtime import ALL_MODES
    plain_argv = _mm_cls_op_argv(tmp_path, golden)
    argv = plain_argv + []
    at = argv.index("INPUT.SIZE")                              # (the KEY VALUE options end the command line)
    argv[at:at] = ["--score-curves", "16"]
    plain = _job(1, plain_argv, tmp_path / "plain")
    one = _job(1, argv, tmp_path / "w1")
    want_tree = sorted(_tree(tmp_path / "plain") + [f"{m}/{n}" for m in ALL_MODES for n in CURVE_FILES])
    assert _tree(tmp_path / "w1") == want_tree, "EVAL_MODE all writes four sets"
    lines, lines0 = _lines(one[0]["stdout"], tmp_path / "w1"), _lines(plain[0]["stdout"], tmp_path / "plain")
    assert [l for l in lines if l not in _curve_lines(lines)] == lines0 and len(_curve_lines(lines)) == 8 and not _curve_lines(lines0)
    for i, l in enumerate(lines):
        if l.startswith("* macro_f1: "):
            assert lines[i + 1].startswith("* mAP: ") and lines[i + 2].startswith("* mean_auroc: "), "the two lines follow the existing ones"
    res, res0 = _job_result(one[0]), _job_result(plain[0])
    assert all(res[k] == v for k, v in res0.items()) and not any("mAP" in k for k in res0)
    assert sorted(k for k in res if k not in res0) == sorted(f"{m}/{k}" for m in ALL_MODES for k in ("mAP", "mean_auroc"))
    for name in _tree(tmp_path / "plain"):
        if name.endswith(".csv"):
            assert (tmp_path / "w1" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes(), name
    hists = {m: torch.load(tmp_path / "w1" / m / "score_hist.pt") for m in ALL_MODES}
    for m, h in hists.items():
        assert (h["lo"], h["hi"], h["bins"]) == (0.0, 1.0, 16) and h["hist"].shape == (4, 2, 19) and h["hist"].dtype == torch.int64
        assert h["hist"][:, 1].sum(dim=1).tolist() == [2, 2, 2, 1] and h["hist"][:, 0].sum(dim=1).tolist() == [5, 5, 5, 6], m
        assert not bool(h["hist"][:, :, [0, 18]].any()), "probabilities: nothing below 0, no NaN"
    for world in (2, 3):
        out = tmp_path / f"w{world}"
        ranks = _job(world, argv, out)
        assert _tree(out) == want_tree
        for m in ALL_MODES:
            for n in CURVE_FILES + ["acc_per_class.csv", "f1_per_class.csv"]:
                assert (out / m / n).read_bytes() == (tmp_path / "w1" / m / n).read_bytes(), (world, m, n)
        assert _lines(ranks[0]["stdout"], out) == lines
        assert [r["results"]["test_shard"]["images"] for r in ranks] == {2: [4, 3], 3: [4, 3, 0]}[world]
        for rank, r in enumerate(ranks):
            assert all(r["results"][k] == res[k] for k in res if "/" in k), (world, rank)
            assert rank == 0 or _lines(r["stdout"], out) == []


def test_runner_zero_shot_trainer_with_a_score_range(golden, tmp_path, capsys):
    from ovmr_amd import cli
    from test_hip_eval_report import _dataset
    spec = synth.SPECS["tiny"]
    R = spec.image_resolution
    root, bpe = _dataset(tmp_path, golden, spec)
    argv = ["--root", str(root), "--seed", "1", "--trainer", "ZeroshotCLIP", "--eval-only", "--clip-weights", str(tmp_path / "clip.pt"),
            "--bpe-path", bpe, "--workers", "0"]
    opts = ["DATASET.NAME", "Caltech101", "INPUT.SIZE", f"({R}, {R})", "DATALOADER.TEST.BATCH_SIZE", "3"]
    with pytest.raises(SystemExit, match="returns logits, which have no natural range"):
        cli.main(argv + ["--score-curves", "--output-dir", str(tmp_path / "x")] + opts)      # (bare: BINS is optional, so not right before the options)
    assert not (tmp_path / "x").exists()
    capsys.readouterr()
    res0 = cli.main(argv + ["--output-dir", str(tmp_path / "plain")] + opts)
    text0 = capsys.readouterr().out
    res = cli.main(argv + ["--output-dir", str(tmp_path / "out"), "--score-curves", "--score-range", "-50", "150"] + opts)
    text = capsys.readouterr().out
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == sorted(["acc_per_class.csv", "f1_per_class.csv"] + CURVE_FILES)
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["acc_per_class.csv", "f1_per_class.csv"]
    keep = lambda t: [l for l in t.splitlines() if l.startswith(("=> ", "* "))]      # noqa: E731
    assert [l for l in keep(text) if l not in _curve_lines(keep(text))] == keep(text0) and len(_curve_lines(keep(text))) == 2
    assert all(res[k] == res0[k] for k in ("accuracy", "error_rate", "macro_f1")) and "mAP" in res and "mAP" not in res0
    h = torch.load(tmp_path / "out" / "score_hist.pt")
    assert (h["lo"], h["hi"], h["bins"]) == (-50.0, 150.0, 256) and h["hist"].shape == (4, 2, 259) and int(h["hist"].sum()) == 7 * 4
    assert h["hist"][:, 1].sum(dim=1).tolist() == [2, 2, 2, 1]
