"""CPU side of the zero-shot trainers (trainers/zsclip.py): the template table, the tokenised ensemble prompts and the runner's refusals,
against tests/golden/zsclip.npz (recorded from the real reference by tests/golden/gen_zsclip.py).  No GPU."""
import gzip

import numpy as np
import pytest


def zsclip_bpe(path, golden):
    """A full-length merge table that tokenises the fixture's ensemble prompts (and tokenizer.npz's texts) as CLIP's own table does: the
    reference's merges those texts reach (bpe_merges.npz and zsclip.npz), each at its own rank, and at every other rank a merge of the
    Euro sign, which stands in for no byte and so never meets a text (test_next_rows_cpu.fixture_bpe)."""
    from ovmr_amd.tokenizer import N_MERGES
    lines = [f"€ {r}" for r in range(N_MERGES)]
    for m in (golden("bpe_merges"), golden("zsclip")):
        for r, pair in zip(m["merge_ranks"], m["merge_pairs"]):
            assert lines[int(r)] in (f"€ {int(r)}", str(pair)), f"rank {int(r)} holds two merges"
            lines[int(r)] = str(pair)
    with gzip.open(path, "wt", encoding="utf-8") as f:
        f.write("#version: fixture\n" + "\n".join(lines) + "\n")


def test_templates_equal_the_reference(golden):
    from ovmr_amd import templates
    g = golden("zsclip")
    assert dict(zip(map(str, g["zs_dataset_names"]), map(str, g["zs_dataset_templates"]))) == templates.DATASET_TEMPLATES
    for ds in ("Caltech101", "ImageNet"):
        assert templates.templates_for("ZeroshotCLIP2", ds) == [str(t) for t in g[f"zs_templates_{ds}"]], ds
    for ds, t in templates.DATASET_TEMPLATES.items():
        assert templates.templates_for("ZeroshotCLIP", ds) == [t]
    assert templates.prompts("a photo of a {}.", ["sea_horse", "yin_yang"]) == ["a photo of a sea horse.", "a photo of a yin yang."]
    assert np.array_equal(np.array([templates.prompts(t, [str(c) for c in g["zs_classnames"]])
                                    for t in templates.templates_for("ZeroshotCLIP2", "Caltech101")]), g["zs_prompts"])


def test_seven_or_eight_templates_and_no_growth():
    from ovmr_amd import templates
    for ds in templates.DATASET_TEMPLATES:
        ts = templates.templates_for("ZeroshotCLIP2", ds)
        assert len(ts) == (7 if ds == "ImageNet" else 8), ds
        assert ts[:7] == list(templates.IMAGENET_TEMPLATES_SELECT)
        if ds != "ImageNet":
            assert ts[7] == templates.DATASET_TEMPLATES[ds]
    first = templates.templates_for("ZeroshotCLIP2", "Caltech101")
    first.append("mutated by the caller {}")
    for _ in range(3):                                  # a second build in the same process sees 8, not 9 (trainers/zsclip.py:83)
        assert len(templates.templates_for("ZeroshotCLIP2", "Caltech101")) == 8
    assert len(templates.IMAGENET_TEMPLATES_SELECT) == 7


@pytest.mark.parametrize("name", ["ImageNet21kP", "", "caltech101"])
def test_unknown_dataset_is_refused_with_the_known_names(name):
    from ovmr_amd import templates
    for trainer in templates.ZEROSHOT_TRAINERS:
        with pytest.raises(KeyError, match="known datasets: .*Caltech101.*ImageNet"):
            templates.templates_for(trainer, name)
    with pytest.raises(ValueError):
        templates.templates_for("MM_CLS_OP", "ImageNet")


def test_bpe_reproduces_the_reference_ids(golden, tmp_path):
    from ovmr_amd import modules
    from ovmr_amd.tokenizer import BPETokenizer
    g = golden("zsclip")
    zsclip_bpe(str(tmp_path / "bpe.txt.gz"), golden)
    tk = BPETokenizer(str(tmp_path / "bpe.txt.gz"))
    prompts = g["zs_prompts"]
    T, C = prompts.shape
    assert (T, C) == (8, 10) and g["zs_token_ids"].shape == (8, 10, 77)
    for t in range(T):
        ids = tk.tokenize([str(p) for p in prompts[t]]).numpy()
        np.testing.assert_array_equal(ids, g["zs_token_ids"][t], err_msg=str(prompts[t][0]))
        np.testing.assert_array_equal(modules.tokenize([str(p) for p in prompts[t]], tk).numpy(), g["zs_token_ids"][t])
    # tokenizer.npz's texts still tokenise as the reference's table does with the merged table
    tg = golden("tokenizer")
    np.testing.assert_array_equal(tk.tokenize([str(t) for t in tg["tok_texts"]]).numpy(), tg["tok_ids"])


def _no_library(monkeypatch):
    from ovmr_amd import checkpoint, runtime

    def boom(*a, **k):
        raise AssertionError("the runner touched the model / library before refusing the job")

    monkeypatch.setattr(runtime, "load_library", boom)
    monkeypatch.setattr(checkpoint, "load_clip_state_dict", boom)


@pytest.mark.parametrize("trainer", ["ZeroshotCLIP", "ZeroshotCLIP2"])
def test_cli_refuses_before_loading_anything(monkeypatch, tmp_path, trainer):
    from ovmr_amd import cli
    _no_library(monkeypatch)
    base = ["--root", str(tmp_path / "nowhere"), "--trainer", trainer, "--eval-only", "--clip-weights", str(tmp_path / "none.pt"),
            "--output-dir", str(tmp_path / "out")]
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process"):
        cli.main(base + ["DATASET.NAME", "Caltech101"])
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(SystemExit, match="ImageNet21kP.*known datasets"):
        cli.main(base + ["DATASET.NAME", "ImageNet21kP"])
    with pytest.raises(SystemExit, match="known datasets"):
        cli.main(base)                                   # DATASET.NAME unset
    with pytest.raises(SystemExit, match="--eval-only"):
        cli.main([a for a in base if a != "--eval-only"] + ["DATASET.NAME", "Caltech101"])
    assert not (tmp_path / "out").exists()


def test_zero_shot_trainers_are_registered():
    from ovmr_amd import trainer
    assert {"MM_CLS_OP", "ZeroshotCLIP", "ZeroshotCLIP2"} <= set(trainer.TRAINER_REGISTRY)
    assert issubclass(trainer.TRAINER_REGISTRY["ZeroshotCLIP2"], trainer.TRAINER_REGISTRY["ZeroshotCLIP"])
    for name in ("ZeroshotCLIP", "ZeroshotCLIP2"):
        cls = trainer.TRAINER_REGISTRY[name]
        for m in ("build_model", "parse_batch_test", "model_inference", "load_model", "test"):
            assert callable(getattr(cls, m)), (name, m)
        with pytest.raises(NotImplementedError):
            cls.train(object.__new__(cls), None)


def test_one_test_loop_pairs_late_outputs_with_their_own_labels(capsys):
    """trainer._EvalTrainer.test() on the host, without an engine: a model that hands batch i's outputs over after batch i + 1 has been
    fetched (two in flight) still has every output counted against its own batch's labels; the split rule; the after-loop hook."""
    from types import SimpleNamespace
    import torch
    from ovmr_amd import modules, trainer
    C = 3
    log = []

    class Late(trainer._EvalTrainer):
        def build_model(self):
            pass

        def outputs(self, inputs):                       # an "image" batch is its rows' predicted classes
            held = None
            for n, x in enumerate(inputs):
                if held is not None:
                    log.append(("output", n - 1))
                    yield held
                held = torch.nn.functional.one_hot(x, C).float()
                last = n
            log.append(("output", last))
            yield held
            log.append("exhausted")

        def after_test(self):
            log.append("after")

    def batches(pred, label, sizes):
        pred, label = torch.tensor(pred).split(sizes), torch.tensor(label).split(sizes)
        return [{"img": p, "label": l} for p, l in zip(pred, label)]

    # 3 + 2 rows; rows 1 and 4 are wrong: 3 of 5.  Batch 1's outputs against batch 0's labels would not even have batch 0's length
    test_loader = batches([0, 2, 2, 1, 1], [0, 1, 2, 1, 0], [3, 2])
    val_loader = batches([2, 1, 0, 0], [2, 1, 0, 1], [2, 2])             # 3 of 4
    cfg = modules.make_cfg(output_dir="")
    cfg.TEST = SimpleNamespace(SPLIT="val")
    for split, val, want, used in (("val", None, 60.0, "test"), ("test", val_loader, 60.0, "test"), ("val", val_loader, 75.0, "val")):
        cfg.TEST.SPLIT = split
        dm = SimpleNamespace(dataset=SimpleNamespace(classnames=["a", "b", "c"]), test_loader=test_loader, val_loader=val)
        t = Late(cfg, dm, device="cpu")
        del log[:]
        capsys.readouterr()
        acc = t.test()
        assert f"Evaluate on the *{used}* set" in capsys.readouterr().out
        assert acc == pytest.approx(want) and acc == list(t.results.values())[0] == t.results["accuracy"]
        assert t.results["error_rate"] == pytest.approx(100.0 - want)
        assert log == [("output", 0), ("output", 1), "exhausted", "after"]
    assert t.test(split="test") == pytest.approx(60.0)                     # an explicit split overrides TEST.SPLIT
    for k in (trainer.MM_CLS_OP, trainer.ZeroshotCLIP, trainer.ZeroshotCLIP2):
        assert k.test is trainer._EvalTrainer.test and k.load_model is trainer._EvalTrainer.load_model
