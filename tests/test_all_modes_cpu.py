"""EVAL_MODE all on the host: the configuration accepts it, the plane order follows runtime.MODES, the test loop keeps one evaluator per
mode -- its prefixed results and the files under OUTPUT_DIR/<mode>/ equal, byte for byte, those of four single-evaluator passes over the
same planes -- and the runner refuses it with --predict before it loads anything."""
import os
from types import SimpleNamespace

import pytest
import torch

C = 7
SIZES = [5, 5, 5, 3]                                        # several batches, a ragged last one


def test_config_accepts_all_and_refuses_unknown_names():
    from ovmr_amd import config
    assert config.setup_cfg(SimpleNamespace(eval_mode="all")).EVAL_MODE == "all"
    assert config.setup_cfg(SimpleNamespace(opts=["EVAL_MODE", "all"])).EVAL_MODE == "all"
    assert config.setup_cfg(SimpleNamespace()).EVAL_MODE == "multimodal"                     # the reference's default stays
    for name in ("text", "vision", "multimodal", "fusion"):
        assert config.setup_cfg(SimpleNamespace(eval_mode=name)).EVAL_MODE == name
    for bad in ("every", "ALL", "fusion,text"):
        with pytest.raises(ValueError, match="EVAL_MODE must be one of"):
            config.setup_cfg(SimpleNamespace(eval_mode=bad))


def test_plane_order_follows_the_mode_values():
    from ovmr_amd import runtime
    assert runtime.ALL_MODES == ("fusion", "text", "vision", "multimodal")
    assert set(runtime.ALL_MODES) == set(runtime.MODES) and [runtime.MODES[m] for m in runtime.ALL_MODES] == [0, 1, 2, 3]
    assert "ovmr_fused_logits_all" in runtime.SIGNATURES


def _planes_and_labels():
    """Four known [N, C] outputs that rank the classes differently (so the four modes' figures differ) and the labels."""
    g = torch.Generator().manual_seed(5)
    n = sum(SIZES)
    labels = torch.randint(0, C - 1, (n,), generator=g)                                      # class C - 1 never occurs as a label
    planes = []
    for p, share in enumerate((0.9, 0.5, 0.7, 0.3)):
        x = torch.rand((n, C), generator=g)
        hit = torch.rand(n, generator=g) < share
        x[torch.arange(n)[hit], labels[hit]] += 2.0 - 0.4 * p
        planes.append(torch.softmax(4 * x, 1))
    return planes, labels


def _trainer(outputs_of, labels, out_dir, topk, **flags):
    from ovmr_amd import modules, trainer

    class StandIn(trainer._EvalTrainer):
        def build_model(self):
            pass

        def outputs(self, inputs):
            for x in inputs:                                 # an "image" batch is its rows' indices
                yield outputs_of(x)

    idx = torch.arange(labels.numel())
    loader = [{"img": i, "label": l} for i, l in zip(idx.split(SIZES), labels.split(SIZES))]
    cfg = modules.make_cfg(output_dir=out_dir)
    cfg.TEST = SimpleNamespace(SPLIT="test", TOPK=topk)
    dm = SimpleNamespace(dataset=SimpleNamespace(classnames=[f"class {c}" for c in range(C)]), test_loader=loader, val_loader=None)
    return StandIn(cfg, dm, device="cpu", **flags)


def _files(d):
    out = {}
    for root, _, names in os.walk(d):
        for n in names:
            with open(os.path.join(root, n), "rb") as f:
                out[os.path.relpath(os.path.join(root, n), d)] = f.read()
    return out


@pytest.mark.parametrize("topk,flags", [(1, {}), (3, {}), (1, dict(per_class_result=True, compute_cmat=True)),
                                        (3, dict(per_class_result=True, compute_cmat=True))],
                         ids=["top1", "top3", "top1-detail", "top3-detail"])
def test_one_pass_equals_four_single_passes(tmp_path, capsys, topk, flags):
    from ovmr_amd import runtime
    planes, labels = _planes_and_labels()
    stacked = torch.stack(planes)                                                            # [4, N, C]
    t = _trainer(lambda x: stacked[:, x], labels, str(tmp_path / "all"), topk, **flags)
    capsys.readouterr()
    first = t.test()
    printed = capsys.readouterr().out
    assert list(t.results)[0] == "fusion/accuracy" and first == t.results["fusion/accuracy"]
    assert len({round(t.results[f"{m}/accuracy"], 6) for m in runtime.ALL_MODES}) == 4, "the four planes were meant to score differently"
    want_keys = ["accuracy", "error_rate", "macro_f1"] + (["perclass_accuracy"] if flags else [])
    assert list(t.results) == [f"{m}/{k}" for m in runtime.ALL_MODES for k in want_keys]
    blocks = printed.split("=> eval mode: ")[1:]
    assert [b.split("\n", 1)[0] for b in blocks] == list(runtime.ALL_MODES)
    summary = [l for l in printed.splitlines() if any(l.startswith(f"=> {m}: accuracy ") for m in runtime.ALL_MODES)]
    assert [l.split(":")[0][3:] for l in summary] == list(runtime.ALL_MODES) and printed.rstrip().splitlines()[-4:] == summary
    for p, mode in enumerate(runtime.ALL_MODES):
        single = _trainer(lambda x, p=p: planes[p][x], labels, str(tmp_path / f"single_{mode}"), topk, **flags)
        capsys.readouterr()
        acc = single.test()
        block = capsys.readouterr().out.split("=> result\n", 1)[1]
        assert {f"{mode}/{k}": v for k, v in single.results.items()} == {k: v for k, v in t.results.items() if k.startswith(mode + "/")}
        assert acc == t.results[f"{mode}/accuracy"]
        mine = blocks[p].split("=> result\n", 1)[1]
        if p == 3:
            mine = mine.rsplit("\n", 5)[0] + "\n"                                            # (the four summary lines follow the last block)
        # the same block, but for the directory in cmat.pt's "saved to" line
        assert mine.replace(os.path.join(str(tmp_path / "all"), mode), "DIR") == block.replace(str(tmp_path / f"single_{mode}"), "DIR")
        got, want = _files(tmp_path / "all" / mode), _files(tmp_path / f"single_{mode}")
        assert sorted(want) == sorted(["acc_per_class.csv", "f1_per_class.csv"] + (["cmat.pt"] if flags else []))
        assert got == want, f"{mode}: files differ"
    assert sorted(os.listdir(tmp_path / "all")) == sorted(runtime.ALL_MODES)                 # nothing beside the four directories
    # a second pass starts from zero, and a two-dimensional model still takes the single evaluator
    assert t.test() == first
    again = _trainer(lambda x: planes[0][x], labels, "", topk, **flags)
    again.test()
    assert "accuracy" in again.results and again.mode_evaluators is None


def test_runner_refuses_predict_with_all(monkeypatch, tmp_path):
    from ovmr_amd import checkpoint, cli, runtime

    def boom(*a, **k):
        raise AssertionError("the runner touched the model / library before refusing the job")

    monkeypatch.setattr(runtime, "load_library", boom)
    monkeypatch.setattr(checkpoint, "load_clip_state_dict", boom)
    (tmp_path / "images").mkdir()
    argv = ["--root", str(tmp_path / "nowhere"), "--trainer", "MM_CLS_OP", "--eval-only", "--clip-weights", str(tmp_path / "none.pt"),
            "--output-dir", str(tmp_path / "out"), "--predict", str(tmp_path / "images")]
    with pytest.raises(SystemExit, match="ONE mode") as e:
        cli.main(argv + ["--eval_mode", "all"])
    assert "\n" not in str(e.value)
    with pytest.raises(SystemExit, match="ONE mode"):
        cli.main(argv + ["EVAL_MODE", "all"])
    with pytest.raises(SystemExit, match="no image file"):                                   # a single mode gets past that check
        cli.main(argv + ["--eval_mode", "fusion"])
    assert not (tmp_path / "out").exists()
