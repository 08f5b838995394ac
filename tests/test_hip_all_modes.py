"""EVAL_MODE all above the kernel: CustomCLIP returns [4, B, C] whose plane p is bit-equal to the model's output under EVAL_MODE =
ALL_MODES[p] (forward, its split form, forward_batches); MM_CLS_OP.test() and the runner report, per mode, the figures and files of that
mode's own run, from one test pass.  tests/test_hip_head_all_modes.py holds the kernel to the single-mode entry point.  Run with -m gpu
on an MI355X."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ovmr_amd import synth

pytestmark = pytest.mark.gpu

SEED = 11


def _pl_state(name="tiny", n_ctx=2):
    return {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(synth.SPECS[name], n_ctx, SEED, True).items()}


def _clip_state(spec):
    return {k: torch.from_numpy(v) for k, v in synth.clip_state_dict(spec, SEED, jitter=True).items()}


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ----------------------------------------------------------------------------- model
def test_model_planes_equal_the_single_modes(tmp_path):
    from ovmr_amd import modules
    from ovmr_amd.runtime import ALL_MODES
    spec = synth.SPECS["tiny"]
    C, S, R = 12, 4, spec.image_resolution
    cm = modules.CLIPModel(_clip_state(spec), spec)
    cfg = modules.make_cfg(n_ctx=2, num_shots=S, eval_mode="all", output_dir=str(tmp_path))
    model = modules.CustomCLIP(cfg, torch.from_numpy(synth.class_token_ids(C, seed=5)), cm, prompt_learner_state=_pl_state(),
                               reserve=(160, 64, 64))
    g = torch.Generator().manual_seed(3)
    labels = torch.arange(C).repeat_interleave(S)
    model.forward_prompt([{"img": torch.randn((C * S, 3, R, R), generator=g), "label": labels}])
    q = torch.randn((160, 3, R, R), generator=g).half().cuda()

    def single_modes(fn):
        outs = []
        for mode in ALL_MODES:
            model.cfg.EVAL_MODE = mode                       # (the existing tests switch the key the same way)
            outs.append(fn())
        model.cfg.EVAL_MODE = "all"
        return outs

    # ---- B = 5: one handle
    got = model(q[:5]).clone()
    assert got.shape == (4, 5, C) and got.dtype == torch.float32 and not hasattr(model, "_split_stream")
    for p, want in enumerate(single_modes(lambda: model(q[:5]).clone())):
        assert want.shape == (5, C) and _bits_equal(got[p], want), f"B = 5, plane {p} ({ALL_MODES[p]})"
    assert len({got[p].cpu().numpy().tobytes() for p in range(4)}) == 4              # four different outputs, not one repeated
    # ---- B = 160: the split forward, each handle writing its rows of every plane
    assert 2 * model.SPLIT_MIN_HALF <= 160 <= model._split_cap() and model._split_keeps_bits(160)
    split = model(q).clone()
    assert hasattr(model, "_split_stream") and split.shape == (4, 160, C)
    for p, want in enumerate(single_modes(lambda: model(q).clone())):
        assert _bits_equal(split[p], want), f"B = 160, plane {p} ({ALL_MODES[p]})"
    model.SPLIT_FORWARD = False
    unsplit = model(q).clone()
    model.SPLIT_FORWARD = True
    assert _bits_equal(unsplit, split)
    assert _bits_equal(split[:, :5], got)                                            # a row does not depend on its batch
    # ---- forward_batches: three batches, a ragged last one, two in flight; resident inputs and a loader that recycles its buffers
    model.OVERLAP_MAX_BATCH = 32
    B = 24
    chunks = [q[0:B], q[B:2 * B], q[2 * B:2 * B + 7]]
    want = [model(c).clone() for c in chunks]
    outs = [o.clone() for o in model.forward_batches(iter(chunks), stable_inputs=True)]
    assert getattr(model, "_twin_engine", None) is not None
    assert [tuple(o.shape) for o in outs] == [(4, B, C), (4, B, C), (4, 7, C)] and all(_bits_equal(a, b) for a, b in zip(outs, want))

    def recycling_loader():
        bufs = [torch.empty((B, 3, R, R), dtype=torch.float16, device="cuda") for _ in range(2)]
        for i, c in enumerate(chunks):
            bufs[i & 1][:c.shape[0]].copy_(c)
            yield bufs[i & 1][:c.shape[0]]
            bufs[i & 1].fill_(float("nan"))

    outs = [o.clone() for o in model.forward_batches(recycling_loader())]
    assert all(_bits_equal(a, b) for a, b in zip(outs, want))
    per_mode = single_modes(lambda: [o.clone() for o in model.forward_batches(iter(chunks), stable_inputs=True)])
    for p in range(4):
        assert all(_bits_equal(w[p], o) for w, o in zip(want, per_mode[p])), f"forward_batches, plane {p}"
    # ---- a ranked prediction needs one mode
    with pytest.raises(ValueError, match="needs one mode"):
        model.predict_topk(q[:5], 2)
    with pytest.raises(ValueError, match="needs one mode"):
        model.predict_topk_batches(iter(chunks), 2)
    model.cfg.EVAL_MODE = "fusion"
    values, indices = model.predict_topk(q[:5], 2)
    assert indices.shape == (5, 2) and torch.equal(indices[:, 0], got[0].argmax(1))


# ----------------------------------------------------------------------------- trainer
def _files(d):
    return {p.relative_to(d).as_posix(): p.read_bytes() for p in sorted(d.rglob("*")) if p.is_file()}


def test_trainer_one_pass_equals_four_trainers(tmp_path, capsys):
    """MM_CLS_OP.test() under EVAL_MODE all against four trainers, one per mode, on the same loaders: TEST.TOPK = 2, both detail flags."""
    from ovmr_amd import modules, trainer
    from ovmr_amd.runtime import ALL_MODES
    from ovmr_amd.tokenizer import BPETokenizer
    from test_next_rows_cpu import make_synthetic_bpe
    spec, S = synth.SPECS["tiny"], 4
    names = ["tench", "gold fish", "sea_horse", "yin yang", "hen", "accordion", "stop sign", "kite", "otter", "lens cap", "llama", "plate"]
    C, R = len(names), spec.image_resolution
    bpe = str(tmp_path / "bpe.txt.gz")
    make_synthetic_bpe(bpe)
    tk = BPETokenizer(bpe)
    labels = np.repeat(np.random.default_rng(1).permutation(C), S)
    img = torch.from_numpy(synth.images(C * S, R, 1234, labels, 0.6))
    tlab = np.arange(31) % C
    timg = torch.from_numpy(synth.images(31, R, 777, tlab, 0.6))
    cuts = [0, 12, 24, 31]                                                          # three test batches, a ragged last one
    dm = SimpleNamespace(dataset=SimpleNamespace(classnames=names), val_loader=None,
                         test_loader=[{"img": timg[a:b], "label": torch.from_numpy(tlab[a:b])} for a, b in zip(cuts[:-1], cuts[1:])],
                         eval_set_loader=[{"img": img[s:s + 4 * S], "label": torch.from_numpy(labels[s:s + 4 * S])} for s in range(0, C * S, 4 * S)])
    clip_sd, pl = _clip_state(spec), _pl_state()

    def run(mode):
        cfg = modules.make_cfg(n_ctx=2, num_shots=S, eval_mode=mode, output_dir=str(tmp_path / mode))
        cfg.TRAINER.NAME = "MM_CLS_OP"
        cfg.TEST = SimpleNamespace(SPLIT="test", TOPK=2)
        t = trainer.build_trainer(cfg, dm, clip_weights=clip_sd, tokenizer=tk, prompt_learner_state=pl, reserve=(16, 64, 64),
                                  per_class_result=True, compute_cmat=True)
        capsys.readouterr()
        acc = t.test()
        return t, acc, capsys.readouterr().out

    t, acc, text = run("all")
    keys = ["accuracy", "error_rate", "macro_f1", "perclass_accuracy"]
    assert list(t.results) == [f"{m}/{k}" for m in ALL_MODES for k in keys] and acc == t.results["fusion/accuracy"]
    out = tmp_path / "all"
    assert sorted(p.name for p in out.iterdir()) == sorted(list(ALL_MODES) + ["mm_classifiers.pt", "visual_tokens.pt"])
    assert [l[len("=> eval mode: "):] for l in text.splitlines() if l.startswith("=> eval mode: ")] == list(ALL_MODES)
    assert [l.split(":")[0][3:] for l in text.rstrip().splitlines()[-4:]] == list(ALL_MODES)
    for mode in ALL_MODES:
        t1, acc1, text1 = run(mode)
        assert {f"{mode}/{k}": v for k, v in t1.results.items()} == {k: v for k, v in t.results.items() if k.startswith(mode + "/")}, mode
        assert acc1 == t.results[f"{mode}/accuracy"]
        single = _files(tmp_path / mode)
        assert sorted(single) == ["acc_per_class.csv", "cmat.pt", "f1_per_class.csv", "mm_classifiers.pt", "visual_tokens.pt"]
        for name in ("acc_per_class.csv", "f1_per_class.csv", "cmat.pt"):
            assert (out / mode / name).read_bytes() == single[name], f"{mode}/{name}"
        assert (out / "mm_classifiers.pt").read_bytes() == single["mm_classifiers.pt"]     # generated once, the same whatever the mode
        block = text1.split("=> result\n", 1)[1].replace(str(tmp_path / mode), "DIR")
        assert block in text.replace(str(out / mode), "DIR"), f"{mode}: the result block differs"


# ----------------------------------------------------------------------------- runner
NAMES = ["accordion", "sea_horse", "stop_sign", "yin_yang"]
PER_CLASS = [2, 2, 2, 1]                                               # seven test images over four classes


def _dataset(tmp_path, golden, spec):
    """Class folders with two PNG exemplars each (train) and seven JPEG test images (val), the BPE fixture, the CLIP weights
    (the job of tests/test_hip_eval_report.py)."""
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
    torch.save(_clip_state(spec), tmp_path / "clip.pt")
    return root, bpe


def test_runner_all_equals_four_runs(golden, tmp_path, capsys):
    from ovmr_amd import checkpoint, cli
    from ovmr_amd.runtime import ALL_MODES
    spec = synth.SPECS["tiny"]
    R = spec.image_resolution
    root, bpe = _dataset(tmp_path, golden, spec)
    checkpoint.save_prompt_learner_state(_pl_state(), str(tmp_path / "ckpt"), 30)
    argv = ["--root", str(root), "--seed", "1", "--trainer", "MM_CLS_OP", "--eval-only", "--clip-weights", str(tmp_path / "clip.pt"),
            "--bpe-path", bpe, "--workers", "2", "--model-dir", str(tmp_path / "ckpt"), "--load-epoch", "30", "--eval_tau", "10", "--n_ctx", "2",
            "--per-class-result", "--confusion-matrix"]
    opts = ["DATASET.NAME", "ImageNet", "INPUT.SIZE", f"({R}, {R})", "DATALOADER.TEST.BATCH_SIZE", "4", "DATASET.NUM_SHOTS", "2"]

    out = tmp_path / "all"
    capsys.readouterr()
    res = cli.main(argv + ["--eval_mode", "all", "--output-dir", str(out)] + opts)
    text = capsys.readouterr().out
    assert sorted(p.name for p in out.iterdir()) == sorted(list(ALL_MODES) + ["mm_classifiers.pt", "visual_tokens.pt"])
    assert [l[len("=> eval mode: "):] for l in text.splitlines() if l.startswith("=> eval mode: ")] == list(ALL_MODES)
    assert res["classnames"] == NAMES and res["pipeline_test"]["images"] == sum(PER_CLASS)
    for mode in ALL_MODES:
        one = tmp_path / mode
        res1 = cli.main(argv + ["--eval_mode", mode, "--output-dir", str(one)] + opts)
        capsys.readouterr()
        for k in ("accuracy", "error_rate", "macro_f1", "perclass_accuracy"):
            assert res[f"{mode}/{k}"] == res1[k], f"{mode}/{k}"
        for name in ("acc_per_class.csv", "f1_per_class.csv", "cmat.pt"):
            assert (out / mode / name).read_bytes() == (one / name).read_bytes(), f"{mode}/{name}"
        assert (out / "mm_classifiers.pt").read_bytes() == (one / "mm_classifiers.pt").read_bytes(), f"mm_classifiers.pt of the {mode} run"
        assert sorted(p.name for p in one.iterdir()) == ["acc_per_class.csv", "cmat.pt", "f1_per_class.csv", "mm_classifiers.pt", "visual_tokens.pt"]
