"""Search by class through the models and the trainer (`pytest -m gpu`), on the tiny synthetic specification: trainer.retrieve /
retrieve_batches over about two dozen images against the host expectation of retrieve_cases.py computed from the concatenated outputs of
forward_batches / inference_batches -- in batches of 4 and of 8, with within_top, with a base, and merged from two halves; then the runner: `--retrieve` in one process against the
call, from --classifiers and from --bank without --root, and as 2 and 3 ranks sharing the GPU over gloo (tests/retrieve_shard_worker.py)
against the one-process file byte for byte.  Exact."""
import csv
import os
import socket
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor, as_completed
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import retrieve_cases as R
from ovmr_amd import synth

pytestmark = pytest.mark.gpu
N_IMAGES = 26


def _floor(out, K):
    from ovmr_amd import runtime
    return runtime.topk_rows(out, K)[0][:, K - 1].cpu()


def _loader(images, B):
    return [{"img": images[a:a + B], "label": torch.zeros(len(images[a:a + B]), dtype=torch.long)} for a in range(0, len(images), B)]


def test_mm_cls_op_trainer_retrieve(tmp_path):
    from ovmr_amd import modules, trainer
    from ovmr_amd.tokenizer import BPETokenizer
    from test_hip_all_modes import _clip_state, _pl_state
    from test_next_rows_cpu import make_synthetic_bpe
    spec, S = synth.SPECS["tiny"], 4
    names = ["tench", "gold fish", "sea_horse", "yin yang", "hen", "accordion", "stop sign"]
    C, Rz = len(names), spec.image_resolution
    bpe = str(tmp_path / "bpe.txt.gz")
    make_synthetic_bpe(bpe)
    labels = np.repeat(np.random.default_rng(1).permutation(C), S)
    img = torch.from_numpy(synth.images(C * S, Rz, 1234, labels, 0.6))
    pool = torch.from_numpy(synth.images(N_IMAGES, Rz, 777, np.arange(N_IMAGES) % C, 0.6))
    dm = SimpleNamespace(dataset=SimpleNamespace(classnames=names), val_loader=None, test_loader=[],
                         eval_set_loader=[{"img": img[s:s + 2 * S], "label": torch.from_numpy(labels[s:s + 2 * S])} for s in range(0, C * S, 2 * S)])
    cfg = modules.make_cfg(n_ctx=2, num_shots=S, eval_mode="fusion", output_dir=str(tmp_path / "out"))
    cfg.TRAINER.NAME = "MM_CLS_OP"
    t = trainer.build_trainer(cfg, dm, clip_weights=_clip_state(spec), tokenizer=BPETokenizer(bpe), prompt_learner_state=_pl_state(),
                              reserve=(16, 64, 64))
    got4 = t.retrieve(_loader(pool, 4), m=5)                  # the first pass generates the classifiers, as test() does
    out = torch.cat([o.clone() for o in t.model.forward_batches(iter([pool[a:a + 8] for a in range(0, N_IMAGES, 8)]))])
    assert out.shape == (N_IMAGES, C) and out.dtype == torch.float32
    want = R.expected(out.cpu(), 5)
    assert got4[0].device.type == "cpu" and R.mismatch(got4, want) is None, R.mismatch(got4, want)
    got8 = t.retrieve(_loader(pool, 8), m=5)
    assert torch.equal(got8[1], got4[1]) and torch.equal(got8[0], got4[0])
    full = t.retrieve(_loader(pool, 8))                       # m = 32 > 26 images: tails of (-1, -inf)
    assert R.mismatch(full, R.expected(out.cpu(), 32)) is None and bool((full[1][:, N_IMAGES:] == -1).all())
    # within_top = 2: the floor is the second-best score of every image
    floor = _floor(out, 2)
    want2 = R.expected(out.cpu(), 5, floor)
    assert R.mismatch(want2, want) is not None
    for B in (4, 8):
        got = t.retrieve(_loader(pool, B), m=5, within_top=2)
        assert R.mismatch(got, want2) is None, (B, R.mismatch(got, want2))
    # two halves with their global bases, merged through the state tensor: what two ranks do
    a = t.model.retrieve_batches(iter([pool[:8]]), 5)
    b = t.model.retrieve_batches(iter([pool[8:16], pool[16:]]), 5, base=8)
    assert R.mismatch(tuple(x.cpu() for x in a.merge(b.state).finish()), want) is None
    for bad, msg in ((dict(m=0), "m must be"), (dict(m=33), "m must be"), (dict(m=5, within_top=C + 1), "within_top must be"),
                     (dict(m=5, base=-1), "base must be")):
        with pytest.raises(ValueError, match="retrieve_batches: " + msg):
            t.model.retrieve_batches(iter([pool[:8]]), **bad)
    t.model.cfg.EVAL_MODE = "all"
    with pytest.raises(ValueError, match="needs one mode"):
        t.retrieve(_loader(pool, 8), m=5)


def test_zeroshot_retrieve_batches(golden, tmp_path):
    from ovmr_amd import modules
    from test_hip_predict import _clip
    g = golden("tiny")
    spec = synth.SPECS["tiny"]
    m = modules.ZeroshotCLIP(_clip(), torch.from_numpy(g["l2_tokenized_prompts"]), reserve=(64, 64, 256))
    C = m.text_features.shape[0]
    pool = torch.from_numpy(synth.images(N_IMAGES, spec.image_resolution, seed=701))
    out = torch.cat([o.clone() for o in m.inference_batches(iter([pool[a:a + 8] for a in range(0, N_IMAGES, 8)]))])
    assert out.dtype == torch.float16 and out.shape == (N_IMAGES, C)
    K = min(2, C)
    for mm in (3, 32):
        want, want2 = R.expected(out.cpu(), mm), R.expected(out.cpu(), mm, _floor(out, K))
        for B in (4, 8):
            batches = [pool[a:a + B] for a in range(0, N_IMAGES, B)]
            got = tuple(x.cpu() for x in m.retrieve_batches(iter(batches), mm).finish())
            assert R.mismatch(got, want) is None, (mm, B, R.mismatch(got, want))
            got = tuple(x.cpu() for x in m.retrieve_batches(iter(batches), mm, within_top=K).finish())
            assert R.mismatch(got, want2) is None, (mm, B, R.mismatch(got, want2))
    top = m.retrieve_batches(iter([]), 3)                     # a rank without a batch: the empty state
    assert not bool(top.state.any()) and bool((top.finish()[1] == -1).all())


# ----------------------------------------------------------------------------- runner
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "retrieve_shard_worker.py")
RANK_LIMIT_S, GROUP_TIMEOUT_S = 300, 120


def _job(world, argv, out):
    """One `--retrieve` job of `world` ranks sharing the one GPU over gloo, OUTPUT_DIR `out` -> what every rank saved
    (tests/retrieve_shard_worker.py).  Every rank is a child under its own time limit; the first that exits non-zero fails the test and
    its peers are stopped."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs, logs = [], []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OVMR_DIST_BACKEND="gloo", OVMR_DIST_TIMEOUT=str(GROUP_TIMEOUT_S), HSA_ENABLE_IPC_MODE_LEGACY="0")
        logs.append(open(f"{out}.rank{rank}.log", "w+"))
        procs.append(subprocess.Popen(["timeout", "-k", "10", str(RANK_LIMIT_S), sys.executable, WORKER, f"{out}.rank{rank}.pt", "--output-dir", str(out)]
                                      + argv, env=env, stdout=logs[-1], stderr=subprocess.STDOUT))
    failed = None
    with ThreadPoolExecutor(max_workers=world) as pool:
        for done in as_completed([pool.submit(lambda r=r: (r, procs[r].wait())) for r in range(world)]):
            rank, code = done.result()
            if code != 0 and failed is None:
                failed = (rank, code)
                for p in procs:
                    if p.poll() is None:
                        p.terminate()
    texts = []
    for f in logs:
        f.seek(0)
        texts.append(f.read())
        f.close()
    if failed is not None:
        pytest.fail(f"rank {failed[0]} of {world} exited with {failed[1]}:\n{texts[failed[0]][-3000:]}", pytrace=False)
    return [torch.load(f"{out}.rank{rank}.pt", weights_only=False) for rank in range(world)]


def _read_retrieval(path):
    rows = list(csv.reader(open(path).read().splitlines()))
    assert rows[0] == ["label", "classname", "rank", "image", "score"]
    return rows[1:]


def _check_retrieval(res_rows, path, want, images, names):
    """The file's lines are the returned rows are the call's (values, indices): class order then rank, unfilled ranks left out."""
    from ovmr_amd import cli
    assert res_rows == cli.retrieval_rows(want[0], want[1], images, names)
    lines = _read_retrieval(path)
    assert len(lines) == len(res_rows) == int((want[1] >= 0).sum())
    for l, r in zip(lines, res_rows):
        assert l == [str(r[0]), r[1], str(r[2]), r[3], repr(r[4])] and float(l[4]) == r[4]
    assert [(int(l[0]), int(l[2])) for l in lines] == sorted((int(l[0]), int(l[2])) for l in lines)


@pytest.mark.timeout(900)
def test_runner_retrieve_zeroshot_one_two_and_three_ranks(golden, tmp_path, capsys):
    """ZeroshotCLIP, a pool of 7 images in batches of 4: two batches, so world 3 has a rank without one.  The one-process file equals the
    call on the same decoded images; 2 and 3 ranks write that file byte for byte and every rank returns its rows."""
    from ovmr_amd import cli, modules
    from ovmr_amd.tokenizer import BPETokenizer
    from test_hip_predict import NAMES, _dataset, _decoded_batches
    spec, B = synth.SPECS["tiny"], 4
    Rz = spec.image_resolution
    root, pics, bpe, clip_sd = _dataset(tmp_path, golden, spec)
    images = sorted(str(p) for p in pics.rglob("*.jpg"))
    common = ["--root", str(root), "--seed", "1", "--trainer", "ZeroshotCLIP", "--eval-only", "--clip-weights", str(tmp_path / "clip.pt"),
              "--bpe-path", bpe, "--workers", "2", "--retrieve", str(pics), "--test-split", "no_such_split"]
    opts = ["DATASET.NAME", "Caltech101", "INPUT.SIZE", f"({Rz}, {Rz})", "DATALOADER.TEST.BATCH_SIZE", str(B)]
    model = modules.ZeroshotCLIP.from_classnames(modules.CLIPModel(clip_sd, spec), NAMES, "Caltech101", BPETokenizer(bpe))
    batches = _decoded_batches(images, Rz, B)
    # in this process: the default M = 32 (tails left out of the file), M = 3, and M = 3 within the top 2
    for extra, kw in (([], dict(m=32)), (["--per-class", "3"], dict(m=3)), (["--per-class", "3", "--within-top", "2"], dict(m=3, within_top=2))):
        out = tmp_path / ("out" + "_".join(extra).replace("--", ""))
        capsys.readouterr()
        res = cli.main(common + ["--output-dir", str(out)] + extra + opts)
        text = capsys.readouterr().out
        want = tuple(x.cpu() for x in model.retrieve_batches(iter(batches), **kw).finish())
        assert res["classnames"] == NAMES and res["pipeline_retrieve"]["images"] == 7 and sorted(p.name for p in out.iterdir()) == ["retrieval.csv"]
        _check_retrieval(res["retrieval"], out / "retrieval.csv", want, images, NAMES)
        assert len([l for l in text.splitlines() if l.startswith("=> the ")]) == 1 and f"of 7 images for each of {len(NAMES)} classes" in text
    assert len(_read_retrieval(tmp_path / "out" / "retrieval.csv")) == 7 * len(NAMES)
    with pytest.raises(SystemExit, match=r"--within-top 5: K must lie in \[1, min\(32, 4 classes\)\]"):
        cli.main(common + ["--output-dir", str(tmp_path / "x"), "--within-top", "5"] + opts)
    # as child processes: one rank, then two and three over gloo
    argv = common + ["--per-class", "3"] + opts
    one = _job(1, argv, tmp_path / "w1")
    first = (tmp_path / "w1" / "retrieval.csv").read_bytes()
    assert first == (tmp_path / "outper-class_3" / "retrieval.csv").read_bytes() and one[0]["test_shard"] is None
    for world in (2, 3):
        ranks = _job(world, argv, tmp_path / f"w{world}")
        assert sorted(p.name for p in (tmp_path / f"w{world}").iterdir()) == ["retrieval.csv"]
        assert (tmp_path / f"w{world}" / "retrieval.csv").read_bytes() == first, world
        assert [r["test_shard"]["images"] for r in ranks] == {2: [4, 3], 3: [4, 3, 0]}[world]
        for rank, r in enumerate(ranks):
            assert r["retrieval"] == one[0]["retrieval"], (world, rank)
            assert ("=> the 3 best" in r["stdout"]) == (rank == 0)


@pytest.mark.timeout(900)
def test_runner_retrieve_mm_cls_op_bank_classifiers_ranks_and_predict(golden, tmp_path):
    """MM_CLS_OP: after a generation (which also saves the bank), from --classifiers, from --bank without --root, and as two ranks -- one
    retrieval.csv, byte for byte.  --predict on the same folder writes the predictions.csv it wrote before and after."""
    from ovmr_amd import checkpoint, cli, config, modules
    from ovmr_amd.tokenizer import BPETokenizer
    from test_hip_predict import NAMES, _check_csv, _dataset, _decoded_batches, _pl_state
    spec, B, S = synth.SPECS["tiny"], 4, 2
    Rz = spec.image_resolution
    root, pics, bpe, clip_sd = _dataset(tmp_path, golden, spec)
    images = sorted(str(p) for p in pics.rglob("*.jpg"))
    checkpoint.save_prompt_learner_state(_pl_state(), str(tmp_path / "ckpt"), 30)
    model_args = ["--seed", "1", "--trainer", "MM_CLS_OP", "--eval-only", "--clip-weights", str(tmp_path / "clip.pt"), "--bpe-path", bpe,
                  "--model-dir", str(tmp_path / "ckpt"), "--load-epoch", "30", "--eval_mode", "fusion", "--eval_tau", "10", "--n_ctx", "2", "--workers", "2"]
    search = ["--retrieve", str(pics), "--per-class", "5", "--within-top", "2"]
    opts = ["DATASET.NAME", "ImageNet", "INPUT.SIZE", f"({Rz}, {Rz})", "DATALOADER.TEST.BATCH_SIZE", str(B), "DATASET.NUM_SHOTS", str(S)]
    out = tmp_path / "out"
    before = cli.main(["--root", str(root)] + model_args + ["--predict", str(pics), "--topk", "2", "--output-dir", str(tmp_path / "p0")] + opts)
    res = cli.main(["--root", str(root)] + model_args + search + ["--save-bank", "--output-dir", str(out)] + opts)
    assert sorted(p.name for p in out.iterdir()) == ["mm_classifiers.pt", "reference_bank.pt", "retrieval.csv", "visual_tokens.pt"]
    assert res["pipeline_exemplar"]["images"] == len(NAMES) * S and res["pipeline_retrieve"]["images"] == 7
    cfg = config.setup_cfg(cli.parse(["--root", str(root)] + model_args + ["--output-dir", str(tmp_path / "unused")] + opts))
    m = modules.CustomCLIP(cfg, NAMES, modules.CLIPModel(clip_sd, spec), tokenizer=BPETokenizer(bpe), prompt_learner_state=_pl_state(), reserve=(B, 256, 1024))
    m.load_classifiers(str(out / "mm_classifiers.pt"))
    want = tuple(x.cpu() for x in m.retrieve_batches(iter(_decoded_batches(images, Rz, B)), 5, within_top=2).finish())
    _check_retrieval(res["retrieval"], out / "retrieval.csv", want, images, NAMES)
    first = (out / "retrieval.csv").read_bytes()
    res2 = cli.main(["--root", str(root)] + model_args + search + ["--classifiers", str(out / "mm_classifiers.pt"), "--output-dir", str(tmp_path / "out2")] + opts)
    assert "pipeline_exemplar" not in res2 and sorted(p.name for p in (tmp_path / "out2").iterdir()) == ["retrieval.csv"]
    assert (tmp_path / "out2" / "retrieval.csv").read_bytes() == first
    res3 = cli.main(model_args + search + ["--bank", str(out / "reference_bank.pt"), "--output-dir", str(tmp_path / "out3")] + opts)      # no --root
    assert "pipeline_exemplar" not in res3 and res3["classnames"] == NAMES and sorted(p.name for p in (tmp_path / "out3").iterdir()) == ["retrieval.csv"]
    assert (tmp_path / "out3" / "retrieval.csv").read_bytes() == first and res3["retrieval"] == res["retrieval"]
    ranks = _job(2, ["--root", str(root)] + model_args + search + opts, tmp_path / "w2")                                                  # generation sharded by class, the pool by batches
    assert (tmp_path / "w2" / "retrieval.csv").read_bytes() == first and [r["test_shard"]["images"] for r in ranks] == [4, 3]
    assert all(r["retrieval"] == res["retrieval"] for r in ranks)
    with pytest.raises(SystemExit, match="--retrieve"):
        cli.main(["--root", str(root)] + model_args + search + ["--predict", str(pics), "--output-dir", str(tmp_path / "x")] + opts)
    # --predict is what it was: the same file before and after the searches, and the file test_hip_predict.py describes
    after = cli.main(["--root", str(root)] + model_args + ["--predict", str(pics), "--topk", "2", "--output-dir", str(tmp_path / "p1")] + opts)
    assert (tmp_path / "p0" / "predictions.csv").read_bytes() == (tmp_path / "p1" / "predictions.csv").read_bytes()
    preds = _check_csv(after, tmp_path / "p1" / "predictions.csv", images, 2, NAMES)
    assert before["predictions"] == after["predictions"]
    probs = torch.cat([m(b) for b in _decoded_batches(images, Rz, B)])
    assert [r[0][0] for _, r in preds] == probs.argmax(1).cpu().tolist()
