"""The linear probe through the model, the trainer and the runner, on the real engine (`pytest -m gpu`): the `tiny` model and the synthetic
folder of tests/test_hip_eval_report.py (four classes, two PNG exemplars each, seven JPEG test images).  The figures of a
`--trainer LinearProbe` run against those computed on the host from the written linear_probe.pt and the model's own features; --probe with
--predict and no --root; --bank against the folder fit, bit for bit; the search's trace against the rule of test_probe_cpu.py; two gloo
ranks against one process."""
import os
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from ovmr_amd import synth

pytestmark = pytest.mark.gpu
SPEC = synth.SPECS["tiny"]
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "probe_shard_worker.py")
B = 4


@pytest.fixture(scope="module")
def job(tmp_path_factory, golden):
    """The data set, the common command line, and the one-process `--probe-c 1` run every test is held against."""
    from test_hip_eval_report import NAMES, _dataset
    from ovmr_amd import cli
    tmp = tmp_path_factory.mktemp("probe")
    root, bpe = _dataset(tmp, golden, SPEC)
    R = SPEC.image_resolution
    common = ["--root", str(root), "--seed", "1", "--eval-only", "--clip-weights", str(tmp / "clip.pt"), "--bpe-path", bpe, "--workers", "2"]
    opts = ["INPUT.SIZE", f"({R}, {R})", "DATASET.NAME", "ImageNet", "DATALOADER.TEST.BATCH_SIZE", str(B), "DATASET.NUM_SHOTS", "2"]
    out = tmp / "fit"
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = cli.main(common + ["--trainer", "LinearProbe", "--probe-c", "1", "--output-dir", str(out)] + opts)
    return dict(tmp=tmp, root=root, common=common, opts=opts, out=out, res=res, printed=buf.getvalue(), names=list(NAMES), bpe=bpe)


def _host_scores(job, state):
    """Scores of the test items on the host: the model's own features (the PIL transform, the runner's batches), W and b of the file, fp64."""
    from PIL import Image
    from ovmr_amd import cli, modules
    clip_sd = torch.load(job["tmp"] / "clip.pt")
    model = modules.LinearProbe(modules.CLIPModel(clip_sd, SPEC), job["names"], reserve=(64, 64, 256))
    _, items = cli.list_split(str(job["root"]), "val")
    R = SPEC.image_resolution
    imgs = torch.stack([cli.test_transform(Image.open(p), R, interpolation="bilinear", mean=None) for p, _ in items])
    feats = torch.cat([model.engine.encode_image(imgs[s:s + B], normalize=True).float().cpu() for s in range(0, len(items), B)])
    return feats.double() @ state.W.double().T + state.b.double(), [l for _, l in items], items


def test_runner_fits_writes_and_evaluates(job):
    from sklearn.metrics import f1_score
    from test_hip_zeroshot import _check_outputs
    from ovmr_amd import probe
    out, res, printed = job["out"], job["res"], job["printed"]
    assert sorted(p.name for p in out.iterdir()) == ["acc_per_class.csv", "f1_per_class.csv", "linear_probe.pt"]
    state = probe.LinearProbeState.read(str(out / "linear_probe.pt"))
    assert state.classnames == job["names"] == res["classnames"] and state.shots.tolist() == [2] * 4 and state.c == 1.0 and state.search is None
    assert state.converged and state.tol == 1e-4 and 1 <= state.n_iter <= 1000 and state.W.shape == (4, SPEC.embed_dim)
    lines = [l for l in printed.splitlines() if l.startswith("=> linear probe:")]
    assert len(lines) == 1 and lines[0].startswith(f"=> linear probe: C 1 iterations {state.n_iter} converged True train loss ")
    assert printed.index("=> linear probe:") < printed.index("* accuracy:")
    scores, y, _ = _host_scores(job, state)
    top = np.sort(scores.numpy(), axis=1)
    print(f"smallest top-two gap of the host scores: {(top[:, -1] - top[:, -2]).min():.3e}")
    pred, y = scores.argmax(dim=1).numpy(), np.asarray(y)                  # (the first of equal scores: the library's tie rule)
    present = np.unique(y)
    want = (100.0 * float((pred == y).mean()), 100.0 * f1_score(y, pred, average="macro", labels=present),
            {str(c): 100.0 * float((pred[y == c] == c).mean()) for c in present}, list(100.0 * f1_score(y, pred, average=None, labels=present)))
    _check_outputs(res, out, want)


def test_probe_file_predicts_without_a_root(job):
    from ovmr_amd import cli, probe
    common = [a for a in job["common"] if a not in ("--root", str(job["root"]))]
    out = job["tmp"] / "predict"
    res = cli.main(common + ["--trainer", "LinearProbe", "--probe", str(job["out"] / "linear_probe.pt"), "--predict", str(job["root"] / "val"),
                             "--topk", "2", "--output-dir", str(out)] + job["opts"])
    assert sorted(p.name for p in out.iterdir()) == ["predictions.csv"], "nothing is fitted, no probe is written"
    scores, _, items = _host_scores(job, probe.LinearProbeState.read(str(job["out"] / "linear_probe.pt")))
    assert [p for p, _ in res["predictions"]] == [p for p, _ in items]
    assert [ranks[0][0] for _, ranks in res["predictions"]] == scores.argmax(dim=1).tolist()
    assert [ranks[0][1] for _, ranks in res["predictions"]] == [job["names"][c] for c in scores.argmax(dim=1).tolist()]
    got = torch.tensor([[r[2] for r in ranks] for _, ranks in res["predictions"]], dtype=torch.float64)
    assert float((got - scores.sort(dim=1, descending=True).values[:, :2]).abs().max()) < 1e-4


def test_bank_fit_equals_the_folder_fit_bit_for_bit(job):
    from test_hip_eval_report import _pl_state
    from ovmr_amd import checkpoint, cli, probe
    tmp = job["tmp"]
    checkpoint.save_prompt_learner_state(_pl_state(), str(tmp / "ckpt"), 30)
    cli.main(job["common"] + ["--trainer", "MM_CLS_OP", "--model-dir", str(tmp / "ckpt"), "--load-epoch", "30", "--eval_mode", "fusion", "--eval_tau",
                              "10", "--n_ctx", "2", "--save-bank", "--output-dir", str(tmp / "mm")] + job["opts"])
    res = cli.main(job["common"] + ["--trainer", "LinearProbe", "--bank", str(tmp / "mm" / "reference_bank.pt"), "--output-dir", str(tmp / "bank")]
                   + job["opts"])
    a, b = (probe.LinearProbeState.read(str(tmp / d / "linear_probe.pt")) for d in ("bank", "fit"))
    assert torch.equal(a.W.view(torch.int32), b.W.view(torch.int32)) and torch.equal(a.b.view(torch.int32), b.b.view(torch.int32))
    assert (a.n_iter, a.converged, a.shots.tolist(), a.classnames) == (b.n_iter, b.converged, b.shots.tolist(), b.classnames)
    assert res["accuracy"] == job["res"]["accuracy"] and "pipeline_exemplar" not in res, "no exemplar is decoded"


def test_search_follows_the_rule_on_its_own_accuracies(job, capsys):
    from ovmr_amd import cli, probe
    root3 = job["tmp"] / "data3"
    shutil.copytree(job["root"], root3)
    shutil.copytree(root3 / "train", root3 / "probeval")
    common = [str(root3) if a == str(job["root"]) else a for a in job["common"]]
    out = job["tmp"] / "search"
    cli.main(common + ["--trainer", "LinearProbe", "--probe-c", "search", "--probe-val-split", "probeval", "--probe-steps", "3", "--output-dir", str(out)]
             + job["opts"])
    state = probe.LinearProbeState.read(str(out / "linear_probe.pt"))
    trace = state.search
    assert len(trace) == 3 and state.c == trace[-1][2] and f"=> linear probe: C {state.c:g} " in capsys.readouterr().out
    assert any(trace[0][:2] == (1e-1 * c, 1e1 * c) for c in probe.SWEEP), "the first bounds: a decade to either side of the sweep's peak"
    for (cl, cr, chosen, acc), nxt in zip(trace, trace[1:] + [None]):
        assert chosen in (cl, cr) and 0.0 <= acc <= 1.0
        if nxt is not None:
            mid = 0.5 * (np.log10(cr) + np.log10(cl))
            want = (np.power(10, mid), np.power(10, np.log10(cr))) if chosen == cr and chosen != cl else (np.power(10, np.log10(cl)), np.power(10, mid))
            assert nxt[:2] == (float(want[0]), float(want[1])), (trace, want)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.timeout(600)
def test_two_ranks_report_the_one_process_figures(job):
    from test_hip_eval_shard import _blocks
    world, out, port = 2, job["tmp"] / "w2", _free_port()
    argv = job["common"] + ["--trainer", "LinearProbe", "--probe-c", "1", "--output-dir", str(out)] + job["opts"]
    procs, logs = [], []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OVMR_DIST_BACKEND="gloo", OVMR_DIST_TIMEOUT="120", HSA_ENABLE_IPC_MODE_LEGACY="0")
        logs.append(open(f"{out}.rank{rank}.log", "w+"))
        procs.append(subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, WORKER, f"{out}.rank{rank}.pt"] + argv, env=env, stdout=logs[-1],
                                      stderr=subprocess.STDOUT))
    codes = [p.wait() for p in procs]
    texts = []
    for f in logs:
        f.seek(0)
        texts.append(f.read())
        f.close()
    assert codes == [0, 0], "\n".join(t[-2000:] for t in texts)
    ranks = [torch.load(f"{out}.rank{rank}.pt", weights_only=False) for rank in range(world)]
    from ovmr_amd import probe
    one = probe.LinearProbeState.read(str(job["out"] / "linear_probe.pt"))
    for r in ranks:                                               # every rank fitted the same probe, to the bit
        assert torch.equal(r["W"].view(torch.int32), one.W.view(torch.int32)) and torch.equal(r["b"].view(torch.int32), one.b.view(torch.int32))
        assert r["n_iter"] == one.n_iter
        for k in ("accuracy", "error_rate", "macro_f1"):
            assert r["results"][k] == job["res"][k]
    assert _blocks(ranks[0]["stdout"], out) == _blocks(job["printed"], job["out"]) and _blocks(ranks[1]["stdout"], out) == []
    assert [r["results"]["test_shard"]["images"] for r in ranks] == [4, 3]
    for name in ("acc_per_class.csv", "f1_per_class.csv"):
        assert (out / name).read_bytes() == (job["out"] / name).read_bytes()
    two = probe.LinearProbeState.read(str(out / "linear_probe.pt"))
    assert torch.equal(two.W, one.W) and torch.equal(two.b, one.b)
