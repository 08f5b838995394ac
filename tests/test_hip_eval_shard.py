"""The runner's test pass sharded over ranks, on the real engine (`pytest -m gpu`): `ovmr_amd.cli.main` as 2 and 3 processes sharing the
test box's one GPU (process group gloo) against the one-process run of the same command line -- results, result blocks, every file under
OUTPUT_DIR -- by equality; nothing here carries a tolerance.  The data set is the synthetic folder of tests/test_hip_eval_report.py (`tiny`
model, four classes, two PNG exemplars each, seven JPEG test images).  Each rank is a child process under its own `timeout`
(tests/eval_shard_worker.py); a dead peer ends the others at OVMR_DIST_TIMEOUT."""
import os
import socket
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor, as_completed

import numpy as np
import pytest
import torch

from ovmr_amd import synth

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "eval_shard_worker.py")
RANK_LIMIT_S, GROUP_TIMEOUT_S = 300, 120
TIMED = ("test_shard", "pipeline_exemplar", "pipeline_test")            # per-rank bookkeeping and wall-clock figures: not the job's result


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _job(world, argv, out, backend="gloo"):
    """One runner job of `world` ranks with OUTPUT_DIR `out` -> [{"results", "stdout"}] per rank.  The ranks start together (they meet in
    collectives); the first rank that exits non-zero fails the test, its peers are stopped and nothing more is launched."""
    port = _free_port()
    procs, logs = [], []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank if backend == "nccl" else 0), WORLD_SIZE=str(world),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OVMR_DIST_BACKEND=backend, OVMR_DIST_TIMEOUT=str(GROUP_TIMEOUT_S),
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        logs.append(open(f"{out}.rank{rank}.log", "w+"))
        procs.append(subprocess.Popen(["timeout", "-k", "10", str(RANK_LIMIT_S), sys.executable, WORKER, f"{out}.rank{rank}.pt", "--output-dir", str(out)] +
                                      argv, env=env, stdout=logs[-1], stderr=subprocess.STDOUT))
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


def _blocks(text, out):
    """The result blocks of a rank's stdout: the `=> ...` headers, the `* ...` figures and cmat.pt's line, OUTPUT_DIR made neutral."""
    return [l.replace(str(out), "OUT") for l in text.splitlines() if l.startswith(("=> ", "* ", "Confusion matrix is saved to"))]


def _tree(out):
    return sorted(os.path.relpath(os.path.join(d, n), out) for d, _, names in os.walk(out) for n in names)


def _job_result(rank_out):
    return {k: v for k, v in rank_out["results"].items() if k not in TIMED}


def _same_as_one_process(one, one_dir, ranks, out, world, n_batches, model_files):
    from ovmr_amd.shard import shard_range
    r0 = ranks[0]
    assert _job_result(r0) == _job_result(one[0]) and list(_job_result(r0)) == list(_job_result(one[0]))
    assert _blocks(r0["stdout"], out) == _blocks(one[0]["stdout"], one_dir) and "=> result" in r0["stdout"]
    assert _tree(out) == _tree(one_dir)
    for name in _tree(out):
        a, b = os.path.join(out, name), os.path.join(one_dir, name)
        if name.endswith(".csv"):
            with open(a, "rb") as fa, open(b, "rb") as fb:
                assert fa.read() == fb.read(), name
        elif name.endswith("cmat.pt"):
            ca, cb = torch.load(a, weights_only=False), torch.load(b, weights_only=False)
            assert isinstance(ca, np.ndarray) and ca.dtype == cb.dtype and ca.shape == cb.shape and np.array_equal(ca, cb), name
        else:
            assert name in model_files, name
            ta, tb = torch.load(a, map_location="cpu"), torch.load(b, map_location="cpu")
            assert sorted(ta) == sorted(tb) and all(ta[k].dtype == tb[k].dtype and torch.equal(ta[k], tb[k]) for k in ta), name
    # every rank holds the job's figures; ranks > 0 print no result block; each image was evaluated on exactly one rank
    for rank, r in enumerate(ranks):
        assert _job_result(r) == _job_result(r0), rank
        shard = r["results"]["test_shard"]
        assert (shard["rank"], shard["world"]) == (rank, world) and tuple(shard["batches"]) == shard_range(n_batches, rank, world)
        if rank:
            assert _blocks(r["stdout"], out) == [], rank
    images = [r["results"]["test_shard"]["images"] for r in ranks]
    assert sum(images) == 7 and images[1] > 0, images
    assert "test_shard" not in one[0]["results"]


def _setup(tmp_path, golden):
    from test_hip_eval_report import _dataset
    spec = synth.SPECS["tiny"]
    root, bpe = _dataset(tmp_path, golden, spec)
    R = spec.image_resolution
    common = ["--root", str(root), "--seed", "1", "--eval-only", "--clip-weights", str(tmp_path / "clip.pt"), "--bpe-path", bpe,
              "--per-class-result", "--confusion-matrix"]
    return common, ["INPUT.SIZE", f"({R}, {R})", "TEST.TOPK", "2"]


def _mm_cls_op_argv(tmp_path, golden):
    from ovmr_amd import checkpoint
    from test_hip_eval_report import _pl_state
    common, opts = _setup(tmp_path, golden)
    checkpoint.save_prompt_learner_state(_pl_state(), str(tmp_path / "ckpt"), 30)
    return common + ["--trainer", "MM_CLS_OP", "--workers", "2", "--model-dir", str(tmp_path / "ckpt"), "--load-epoch", "30", "--eval_mode", "all",
                     "--eval_tau", "10", "--n_ctx", "2"] + opts + ["DATASET.NAME", "ImageNet", "DATALOADER.TEST.BATCH_SIZE", "4",
                                                                  "DATASET.NUM_SHOTS", "2"]


MODEL_FILES = ["mm_classifiers.pt", "visual_tokens.pt"]


@pytest.mark.timeout(900)
def test_mm_cls_op_all_modes_sharded_equals_one_process(golden, tmp_path):
    """--eval_mode all --per-class-result --confusion-matrix, TEST.TOPK 2, test batches of 4: two batches, so world 3 has a rank without
    one.  On the parent commit ranks > 0 return {} and never see the test set."""
    argv = _mm_cls_op_argv(tmp_path, golden)
    one = _job(1, argv, tmp_path / "w1")
    assert len(_tree(tmp_path / "w1")) == 2 + 4 * 3 and "fusion/perclass_accuracy" in one[0]["results"]
    for world in (2, 3):
        ranks = _job(world, argv, tmp_path / f"w{world}")
        _same_as_one_process(one, tmp_path / "w1", ranks, tmp_path / f"w{world}", world, 2, MODEL_FILES)
        assert [r["results"]["test_shard"]["images"] for r in ranks] == {2: [4, 3], 3: [4, 3, 0]}[world]


@pytest.mark.timeout(900)
def test_zero_shot_trainers_sharded_equal_one_process(golden, tmp_path):
    """ZeroshotCLIP with test batches of 2: four batches, world 3 gets 2 / 1 / 1; ZeroshotCLIP2 (the ensembled classifier, computed by every
    rank itself) once, at world 2.  On the parent commit the runner refuses these jobs."""
    common, opts = _setup(tmp_path, golden)
    for trainer, worlds, workers in (("ZeroshotCLIP", (2, 3), "2"), ("ZeroshotCLIP2", (2,), "0")):
        argv = common + ["--trainer", trainer, "--workers", workers] + opts + ["DATASET.NAME", "Caltech101", "DATALOADER.TEST.BATCH_SIZE", "2"]
        one = _job(1, argv, tmp_path / f"{trainer}_w1")
        assert _tree(tmp_path / f"{trainer}_w1") == ["acc_per_class.csv", "cmat.pt", "f1_per_class.csv"]
        for world in worlds:
            out = tmp_path / f"{trainer}_w{world}"
            ranks = _job(world, argv, out)
            _same_as_one_process(one, tmp_path / f"{trainer}_w1", ranks, out, world, 4, [])
            assert [r["results"]["test_shard"]["images"] for r in ranks] == {2: [4, 3], 3: [4, 2, 1]}[world]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs at least 2 GPUs: one RCCL rank per device (armed for the 8-GPU node)")
@pytest.mark.timeout(900)
def test_rccl_one_rank_per_device_sharded_pass_equals_one_process(golden, tmp_path):
    """The MM_CLS_OP job above over `nccl` (= RCCL), one process per GPU, world = min(8, devices): the evaluator state is summed on device
    tensors (shard._staged is the identity for this backend).  Skipped on a one-GPU box, collected there."""
    from ovmr_amd.shard import shard_range
    world = min(8, torch.cuda.device_count())
    argv = _mm_cls_op_argv(tmp_path, golden)
    one = _job(1, argv, tmp_path / "w1")
    ranks = _job(world, argv, tmp_path / "rccl", backend="nccl")
    _same_as_one_process(one, tmp_path / "w1", ranks, tmp_path / "rccl", world, 2, MODEL_FILES)
    spans = [shard_range(2, r, world) for r in range(world)]
    assert [r["results"]["test_shard"]["images"] for r in ranks] == [min(7, 4 * b) - min(7, 4 * a) for a, b in spans]
