"""Exact ranking figures through the evaluator and the runner (`pytest -m gpu`): Classification(exact=True) on the device against the
host evaluator on the same outputs, then the synthetic-folder job of tests/test_hip_eval_report.py with `--exact-curves` -- in one
process, and as 2 and 3 ranks sharing the GPU over gloo (tests/eval_shard_worker.py; seven test images in batches of 4: a count the world
sizes do not divide, and at world 3 a rank without an image) -- whose rank files must be byte-equal across the three runs; and a
zero-shot trainer, which needs no range, against sklearn on the outputs it produced."""
import csv
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import ranks_cases as K
from ovmr_amd import synth

pytestmark = pytest.mark.gpu
RANK_FILES = ["rank_state.pt", "ranks_per_class.csv"]


@pytest.mark.parametrize("kind", ["probs", "logits"])
def test_device_evaluator_equals_host(tmp_path, kind, monkeypatch):
    from ovmr_amd import runtime
    from ovmr_amd.evaluator import Classification
    from test_hip_eval_report import C, CUTS, _outputs
    mo, gt = _outputs(kind)
    sp = torch.from_numpy(K.specials(mo.dtype == torch.float16)).to(mo.dtype)
    at = torch.randperm(mo.numel(), generator=torch.Generator().manual_seed(1))[:4 * len(sp)]
    mo.view(-1)[at] = sp.repeat(4)                              # NaN, infinities, both zeros, denormals: among positives and negatives
    mo[torch.arange(0, 40), gt[:40]] = sp.repeat(3)[:40]
    launches = []
    real = runtime.eval_ranks
    monkeypatch.setattr(runtime, "eval_ranks", lambda *a, **k: (launches.append(a[0].shape[0]), real(*a, **k))[1])
    got = {}
    for device in ("cuda", "cpu"):
        ev = Classification(C, [f"class {i}" for i in range(C)], device=device, per_class=device == "cuda", exact=True)
        before = len(launches)
        for a, b in zip(CUTS[:-1], CUTS[1:]):
            ev.process(mo[a:b].to(device), gt[a:b].to(device))
        assert len(ev._kept) == 3 and ev._kept[0][0].dtype == mo.dtype and ev._kept[0][0].device.type == device
        assert len(launches) == before, "nothing is counted before the pass ends"
        buf = io.StringIO()
        with redirect_stdout(buf):
            res = ev.evaluate(str(tmp_path / device))
        got[device] = (ev, res, [l for l in buf.getvalue().splitlines() if l.startswith("* exact_")])
    assert launches == [256, 256, 37], "one launch per kept batch, at the end of the pass, on the device only"
    dev, host = got["cuda"][0], got["cpu"][0]
    assert dev._rank[2].is_cuda and dev._rank[2].dtype == torch.int32 and dev._kept == []
    for a, b in zip(dev.rank_state, host.rank_state):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    edges, estart = K.edges_of(mo, gt, C)
    assert dev.rank_state[0].numpy().view(np.uint32).tolist() == edges.view(np.uint32).tolist() and dev.rank_state[1].tolist() == estart.tolist()
    assert K.mismatch(dev.rank_state[2], K.expected(mo, gt, edges, estart)) is None
    assert int(dev.rank_state[2].sum()) == CUTS[-1] * C and int(dev.rank_state[2][1].sum()) == CUTS[-1]
    assert got["cuda"][1]["exact_mAP"] == got["cpu"][1]["exact_mAP"] and got["cuda"][1]["exact_mean_auroc"] == got["cpu"][1]["exact_mean_auroc"]
    assert got["cuda"][2] == got["cpu"][2] and len(got["cuda"][2]) == 2
    for k in dev.ranks:
        assert np.array_equal(dev.ranks[k], host.ranks[k], equal_nan=True), k
    for name in RANK_FILES:
        assert (tmp_path / "cuda" / name).read_bytes() == (tmp_path / "cpu" / name).read_bytes(), name
    rows = list(csv.reader(open(tmp_path / "cuda" / "ranks_per_class.csv")))
    assert len(rows) == 1 + C and rows[100][2:] == ["0", str(CUTS[-1])] + [""] * 6, "class 99 is never a label"


def _lines(text, out):
    from test_hip_eval_shard import _blocks
    return _blocks(text, out)


@pytest.mark.timeout(900)
def test_runner_all_modes_one_two_and_three_ranks(golden, tmp_path):
    from test_hip_eval_shard import _job, _job_result, _mm_cls_op_argv, _tree
    from ovmr_amd.runtime import ALL_MODES
    argv = _mm_cls_op_argv(tmp_path, golden)
    at = argv.index("INPUT.SIZE")                              # (the KEY VALUE options end the command line)
    argv[at:at] = ["--exact-curves"]
    one = _job(1, argv, tmp_path / "w1")
    tree = _tree(tmp_path / "w1")
    assert [n for n in tree if n.split("/")[-1] in RANK_FILES] == sorted(f"{m}/{n}" for m in ALL_MODES for n in RANK_FILES), "EVAL_MODE all writes four sets"
    lines = _lines(one[0]["stdout"], tmp_path / "w1")
    exact = [l for l in lines if l.startswith("* exact_")]
    assert len(exact) == 8
    for i, l in enumerate(lines):
        if l.startswith("* macro_f1: "):
            assert lines[i + 1].startswith("* exact_mAP: ") and lines[i + 2].startswith("* exact_mean_auroc: "), "the two lines follow the existing ones"
    res = _job_result(one[0])
    assert sorted(k for k in res if "exact" in k) == sorted(f"{m}/{k}" for m in ALL_MODES for k in ("exact_mAP", "exact_mean_auroc"))
    for m in ALL_MODES:
        s = torch.load(tmp_path / "w1" / m / "rank_state.pt")
        E = int(s["estart"][-1])
        assert s["classnames"] == ["accordion", "sea_horse", "stop_sign", "yin_yang"] and s["state"].shape == (2, 2 * E + 4) and 4 <= E <= 7
        assert int(s["state"][1].sum()) == 7 and int(s["state"][0].sum()) == 21 and not bool(s["state"][1, [2 * int(s["estart"][c]) + c for c in range(4)]].any())
        rows = list(csv.reader(open(tmp_path / "w1" / m / "ranks_per_class.csv")))
        assert [r[2:4] for r in rows[1:]] == [["2", "5"], ["2", "5"], ["2", "5"], ["1", "6"]]
    for world in (2, 3):
        out = tmp_path / f"w{world}"
        ranks = _job(world, argv, out)
        assert _tree(out) == tree
        for m in ALL_MODES:
            for n in RANK_FILES + ["acc_per_class.csv", "f1_per_class.csv"]:
                assert (out / m / n).read_bytes() == (tmp_path / "w1" / m / n).read_bytes(), (world, m, n)
        assert _lines(ranks[0]["stdout"], out) == lines
        assert [r["results"]["test_shard"]["images"] for r in ranks] == {2: [4, 3], 3: [4, 3, 0]}[world]
        for rank, r in enumerate(ranks):
            assert all(r["results"][k] == res[k] for k in res if "/" in k), (world, rank)
            assert rank == 0 or _lines(r["stdout"], out) == []


def test_runner_zero_shot_trainer_needs_no_range_and_equals_sklearn(golden, tmp_path, capsys, monkeypatch):
    from sklearn.metrics import average_precision_score, precision_recall_curve, roc_auc_score
    from ovmr_amd import cli
    from ovmr_amd.evaluator import Classification
    from test_hip_eval_report import _dataset
    spec = synth.SPECS["tiny"]
    R = spec.image_resolution
    root, bpe = _dataset(tmp_path, golden, spec)
    argv = ["--root", str(root), "--seed", "1", "--trainer", "ZeroshotCLIP", "--eval-only", "--clip-weights", str(tmp_path / "clip.pt"),
            "--bpe-path", bpe, "--workers", "0"]
    opts = ["DATASET.NAME", "Caltech101", "INPUT.SIZE", f"({R}, {R})", "DATALOADER.TEST.BATCH_SIZE", "3"]
    res0 = cli.main(argv + ["--output-dir", str(tmp_path / "plain")] + opts)
    text0 = capsys.readouterr().out
    dumped = []
    real = Classification.process
    monkeypatch.setattr(Classification, "process", lambda self, mo, gt, *a, **k: (dumped.append((mo.detach().cpu().clone(), gt.cpu().clone())),
                                                                                  real(self, mo, gt, *a, **k))[1])
    res = cli.main(argv + ["--output-dir", str(tmp_path / "out"), "--exact-curves"] + opts)
    text = capsys.readouterr().out
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == sorted(["acc_per_class.csv", "f1_per_class.csv"] + RANK_FILES)
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["acc_per_class.csv", "f1_per_class.csv"]
    keep = lambda t: [l for l in t.splitlines() if l.startswith(("=> ", "* "))]      # noqa: E731
    assert [l for l in keep(text) if not l.startswith("* exact_")] == keep(text0) and len([l for l in keep(text) if l.startswith("* exact_")]) == 2
    assert all(res[k] == res0[k] for k in res0) and sorted(set(res) - set(res0)) == ["exact_mAP", "exact_mean_auroc"]
    mo, y = torch.cat([d[0] for d in dumped]).double().numpy(), torch.cat([d[1] for d in dumped]).numpy()
    assert mo.shape == (7, 4) and dumped[0][0].dtype == torch.float16, "logits, as the trainer returns them"
    rows = list(csv.reader(open(tmp_path / "out" / "ranks_per_class.csv")))
    aps, aucs = [], []
    for c in range(4):
        t, s = (y == c).astype(int), mo[:, c]
        p, r, thr = precision_recall_curve(t, s)
        want = [average_precision_score(t, s), roc_auc_score(t, s), (2 * p * r / np.maximum(p + r, 1e-300)).max()]
        assert rows[1 + c][2:4] == [str(t.sum()), str(7 - t.sum())]
        assert np.abs(np.array([float(v) for v in rows[1 + c][4:7]]) - np.array(want)).max() <= 1e-12, (c, rows[1 + c], want)
        assert float(rows[1 + c][7]) in s[t == 1]
        aps.append(want[0]), aucs.append(want[1])
    assert abs(res["exact_mAP"] - 100 * np.mean(aps)) <= 1e-10 and abs(res["exact_mean_auroc"] - np.mean(aucs)) <= 1e-12
