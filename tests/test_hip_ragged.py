"""Ragged exemplar sets on the HIP path: every class uses exactly the images it has (ovmr_generate_tokens_ragged, PromptLearner.forward
with shots=, CustomCLIP.forward_prompt on a loader whose batches carry "shots").  The contract (include/ovmr_hip.h): per class, the
visual tokens are bit-identical to the uniform entry point run on that class alone with S = shots[c]; the reference's arithmetic is
its own PromptLearner.forward at num_ins = shots[c] (trainers/mm_classifier_one_prompt.py:167-169).  Both entry points end in one
generator over one sequence table (AggSeqs, csrc/common.h): the uniform call is the table's arithmetic mode, and its chunks come from
the same planner.  Needs an MI355X: `pytest -m gpu`.
"""
import numpy as np
import pytest
import torch

from conftest import COS_TOL, assert_cosine, near_tie_classes
from ovmr_amd import synth

pytestmark = pytest.mark.gpu
SEED = 11
SHOTS = [1, 2, 5, 16, 64, 126, 3, 1]          # one image, the uniform default, n_ctx + shots = 128 (the LDS limit), short ones behind it


@pytest.fixture(scope="module")
def O():
    from oracle import ovmr_oracle
    return ovmr_oracle


def _engine(name, n_ctx=2, reserve=(64, 64, 256)):
    from ovmr_amd import modules
    spec = synth.SPECS[name]
    sd = {k: torch.from_numpy(v) for k, v in synth.clip_state_dict(spec, SEED, jitter=True).items()}
    e = modules.CLIPModel(sd, spec).engine(n_ctx)
    e.load_state_dict({}, {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, n_ctx, SEED, True).items()})
    e._pl_loaded = True
    e.finalize(*reserve)
    return e


def _feats(spec, shots, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(sum(shots), spec.embed_dim, generator=g), dim=-1).half()


def _split(feats, shots):
    return list(torch.split(feats, list(shots)))


@pytest.fixture(scope="module")
def small_case():
    """The `small` engine, the packed features of SHOTS and the ragged call's tokens: computed once, shared, left unchanged."""
    e = _engine("small")
    feats = _feats(synth.SPECS["small"], SHOTS, 21).cuda()
    tokens = e.generate_tokens_ragged(feats, SHOTS)
    torch.cuda.synchronize()
    return e, feats, tokens


def test_ragged_tokens_equal_each_class_alone(small_case):
    e, feats, tokens = small_case
    assert tokens.shape == (len(SHOTS), 2, synth.SPECS["small"].embed_dim) and tokens.dtype == torch.float32
    for c, rows in enumerate(_split(feats, SHOTS)):
        alone = e.generate_tokens(rows.unsqueeze(0).contiguous())
        assert torch.equal(tokens[c].view(torch.int32), alone[0].view(torch.int32)), f"class {c} ({SHOTS[c]} shots) != the uniform call on it alone"


def test_ragged_tokens_vs_oracle(O, small_case):
    """The reference's aggregator on each class's own tokens, cat([cls_token, feats_c]) at num_ins = shots[c] (:167-169): the
    tolerances of test_config_c4_sixty_four_shots."""
    e, feats, tokens = small_case
    spec = synth.SPECS["small"]
    pl = {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, 2, SEED, True).items()}
    for c, rows in enumerate(_split(feats.cpu(), SHOTS)):
        with torch.no_grad():
            x = torch.cat([pl["cls_token"], rows.float()], dim=0).unsqueeze(0)
            ref = O.transformer(x, pl, "aggregator.resblocks.", spec.embed_dim // 64, None)[:, :2]
        np.testing.assert_allclose(tokens[c].cpu().numpy(), ref[0].numpy(), atol=5e-4, rtol=1e-3, err_msg=f"class {c}")


def test_ragged_chunks_do_not_change_a_bit(small_case):
    """finalize(max_classes = 3): the aggregator's workspace holds 3 * (2 + 32) = 102 rows, so the call runs as [1, 2, 5, 16, 64]
    (98 rows), [126] alone (128 rows: at least one class per chunk) and [3, 1] -- three chunks, the second ending behind the 128-row
    class."""
    e, feats, tokens = small_case
    e3 = _engine("small", reserve=(64, 64, 3))
    got = e3.generate_tokens_ragged(feats, SHOTS)
    assert torch.equal(got.view(torch.int32), tokens.view(torch.int32))


@pytest.fixture(scope="module")
def one_class_engine():
    """finalize(max_classes = 1): the aggregator's workspace holds 1 * (2 + 32) = 34 rows."""
    return _engine("small", reserve=(64, 64, 1))


@pytest.mark.parametrize("Cb,S", [(7, 3), (3, 32)])
def test_uniform_chunks_do_not_change_a_bit(O, small_case, one_class_engine, Cb, S):
    """The uniform call through the shared chunk planner, 34 aggregator rows: 7 classes x 3 shots run as 6 + 1 classes (floor(34 / 5)
    per chunk), 3 classes x 32 shots one class per chunk (n_ctx + shots = the capacity).  Bit-equal to the default engine's one chunk;
    class 0 against the reference's aggregator within the tolerances of test_ragged_tokens_vs_oracle."""
    spec = synth.SPECS["small"]
    feats = _feats(spec, [S] * Cb, 200 + S).cuda().view(Cb, S, -1)
    got = one_class_engine.generate_tokens(feats)
    one_chunk = small_case[0].generate_tokens(feats)
    torch.cuda.synchronize()
    assert got.shape == (Cb, 2, spec.embed_dim)
    assert torch.equal(got.view(torch.int32), one_chunk.view(torch.int32))
    pl = {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, 2, SEED, True).items()}
    with torch.no_grad():
        x = torch.cat([pl["cls_token"], feats[0].float().cpu()], dim=0).unsqueeze(0)
        ref = O.transformer(x, pl, "aggregator.resblocks.", spec.embed_dim // 64, None)[:, :2]
    np.testing.assert_allclose(got[0].cpu().numpy(), ref[0].numpy(), atol=5e-4, rtol=1e-3)


@pytest.mark.parametrize("S", [1, 16, 33])
def test_all_equal_shots_equal_the_uniform_call(small_case, S):
    e = small_case[0]
    Cb = 9
    feats = _feats(synth.SPECS["small"], [S] * Cb, 100 + S).cuda()
    assert torch.equal(e.generate_tokens_ragged(feats, [S] * Cb), e.generate_tokens(feats.view(Cb, S, -1)))


def test_ragged_refusals_launch_nothing(small_case):
    from ovmr_amd.runtime import OvmrError
    e = small_case[0]
    D = synth.SPECS["small"].embed_dim
    feats = _feats(synth.SPECS["small"], [140], 5).cuda()

    def refused(shots, rows, match):
        import ctypes
        from ovmr_amd.runtime import _ptr, _stream
        out = torch.empty((len(shots), 2, D), device="cuda")
        out.view(torch.int32).fill_(0x5A5A5A5A)
        host = (ctypes.c_int32 * len(shots))(*shots)
        offsets = torch.tensor(np.concatenate([[0], np.cumsum(shots)]), dtype=torch.int32, device="cuda")
        rc = e.lib.ovmr_generate_tokens_ragged(e.h, _ptr(feats), host, _ptr(offsets), len(shots), rows, _ptr(out), _stream())
        torch.cuda.synchronize()
        assert rc == -2 and match in e.lib.ovmr_last_error(e.h).decode()
        assert bool((out.view(torch.int32) == 0x5A5A5A5A).all()), "a refused call wrote tokens"

    refused([3, 0, 4], 7, "class 1")
    refused([3, 127], 130, "class 1")
    refused([3, 4], 8, "add up")
    with pytest.raises(OvmrError, match="exceeds 128"):
        e.generate_tokens_ragged(feats[:130], [3, 127])
    assert e.generate_tokens_ragged(feats[:0], []).shape == (0, 2, D)


@pytest.mark.parametrize("n_ctx", [1, 4])
def test_ragged_tokens_other_context_lengths(O, n_ctx):
    spec, shots = synth.SPECS["tiny"], [1, 7, 128 - n_ctx, 2]
    e = _engine("tiny", n_ctx)
    feats = _feats(spec, shots, 40 + n_ctx).cuda()
    tokens = e.generate_tokens_ragged(feats, shots)
    pl = {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, n_ctx, SEED, True).items()}
    for c, rows in enumerate(_split(feats, shots)):
        assert torch.equal(tokens[c], e.generate_tokens(rows.unsqueeze(0).contiguous())[0]), f"class {c}"
        with torch.no_grad():
            x = torch.cat([pl["cls_token"], rows.float().cpu()], dim=0).unsqueeze(0)
            ref = O.transformer(x, pl, "aggregator.resblocks.", spec.embed_dim // 64, None)[:, :n_ctx]
        np.testing.assert_allclose(tokens[c].cpu().numpy(), ref[0].numpy(), atol=5e-4, rtol=1e-3, err_msg=f"class {c}")


# ---- forward_prompt on a ragged loader ------------------------------------------------------------------------------------------
C_JOB, CYCLE, CAP, IMG_SEED, TOK_SEED = 24, (1, 3, 8, 16), 16, 2, 4      # the seeds: see test_forward_prompt_ragged_vs_oracle
JOB_SHOTS = [CYCLE[c % len(CYCLE)] for c in range(C_JOB)]          # 168 rows


def _job_inputs():
    spec = synth.SPECS["small"]
    labels = np.repeat(np.arange(C_JOB), JOB_SHOTS)
    img = torch.from_numpy(synth.images(len(labels), spec.image_resolution, IMG_SEED, labels, 0.9))
    tok = torch.from_numpy(synth.class_token_ids(C_JOB, seed=TOK_SEED))
    pl = {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, 2, SEED, True).items()}
    return spec, labels, img, tok, pl


def _oracle_ragged(O, img, labels, shots_of, tok, sd, pl, n_ctx=2, tau=10.0):
    """The reference's generation for classes with their own counts, composed per shot-count group from the unchanged oracle
    functions: prompt_learner_forward at num_ins = S for the classes with S rows, get_mm_v_feats on their prompts, and
    multiclass_f1_per_class over ALL rows with their per-row labels (n_label[c] = shots[c] by construction).  labels: the class of
    every row, class after class; shots_of: {class: rows}."""
    C, D = tok.shape[0], sd["visual.proj"].shape[1]
    with torch.no_grad():
        feats = O.l2_normalize(O.encode_image(img.half(), sd))
        prompt_tokens = O.prompt_embeddings(tok, sd)
        vtemp = O.prompt_embeddings(torch.from_numpy(synth.template_token_ids(tok.shape[1])), sd)
        text = O.zero_shot_classifier(tok, sd)
        mm, v = torch.zeros(C, D, dtype=torch.float16), torch.zeros(C, D, dtype=torch.float16)
        tokens = torch.zeros(C, n_ctx, D, dtype=torch.float16)
        row0 = {}
        for r, c in enumerate(labels.tolist()):
            row0.setdefault(c, r)
        for S in sorted(set(shots_of.values())):
            cls = torch.tensor([c for c in shots_of if shots_of[c] == S])
            f = torch.stack([feats[row0[int(c)]:row0[int(c)] + S] for c in cls])
            mm_p, mm_l, v_p, v_l, tk = O.prompt_learner_forward(f, cls, tok[cls].argmax(-1), prompt_tokens, vtemp, pl, n_ctx)
            m_, v_ = O.get_mm_v_feats(mm_p, mm_l, v_p, v_l, sd)
            mm[cls], v[cls], tokens[cls] = m_.half(), v_.half(), tk.half()
        ls = sd["logit_scale"].float().exp()
        row_labels = torch.from_numpy(np.asarray(labels))
        logits = [O.cross_validation_logits(feats.unsqueeze(0), clf, ls) for clf in (mm, v, text.half())]
        f1 = torch.stack([O.multiclass_f1_per_class(lg, row_labels, C) for lg in logits], -1).float()
    return {"mm": mm.float(), "v": v.float(), "t": text.float(), "tokens": tokens, "feats": feats, "logits": logits,
            "fusion_weight": (tau * f1).softmax(-1)}


def _free_of_near_ties(r, C):
    affected = set()
    for lg in r["logits"]:
        affected |= near_tie_classes(lg.float().numpy(), 0.26)
    return np.array([c not in affected for c in range(C)])


def _check_against_oracle(O, model, r, shots, what):
    C, R = len(shots), sum(shots)
    assert_cosine(model.mm_classifier.float().cpu().numpy(), r["mm"].numpy(), COS_TOL, f"{what}: mm")
    assert_cosine(model.visual_classifer.float().cpu().numpy(), r["v"].numpy(), COS_TOL, f"{what}: vision")
    assert_cosine(model.zero_shot_classifier.float().cpu().numpy(), r["t"].numpy(), COS_TOL, f"{what}: text")
    assert_cosine(model.visual_tokens.float().cpu().numpy(), r["tokens"].float().numpy(), COS_TOL, f"{what}: visual_tokens")
    counts, fw = model.xval_counts.cpu(), model.fusion_weight.cpu()
    assert counts[:, 1].sum(-1).tolist() == [R, R, R], f"{what}: every row votes once per classifier"
    assert bool((counts[:, 0] <= torch.tensor(shots)).all()), f"{what}: tp[c] <= shots[c]"
    f1 = torch.stack([O.f1_from_counts(counts[m, 0], counts[m, 1], torch.tensor(shots)) for m in range(3)], -1)
    np.testing.assert_allclose(fw.numpy(), (10.0 * f1).softmax(-1).numpy(), atol=1e-6)
    return fw


def test_forward_prompt_ragged_vs_oracle(O):
    """24 classes of the `small` model with 1, 3, 8, 16, 1, 3, ... exemplars through CustomCLIP.forward_prompt on a ragged loader
    (whole classes per batch, at most 40 rows), against the oracle composed per shot-count group; then the SAME items filled up to 16
    per class by layout_exemplars: other vote totals and another n_label -- the mode is not a relabelled fill."""
    from ovmr_amd import cli, modules
    from ovmr_amd.data import ResidentEvalSet, ResidentRaggedSet
    from test_hip_parity import _clip, _oracle_sd
    spec, labels, img, tok, pl = _job_inputs()
    R = len(labels)
    cm = _clip("small")
    cfg = modules.make_cfg(n_ctx=2, num_shots=CAP, output_dir="", test_batch_size=40)
    model = modules.CustomCLIP(cfg, tok, cm, prompt_learner_state=pl, reserve=(64, 64, 256))
    loader = ResidentRaggedSet(img, labels, 40, num_classes=C_JOB)
    assert loader.shots.tolist() == JOB_SHOTS and max(b - a for a, b, _ in loader.spans) <= 40 and len(loader) > 4
    model.forward_prompt(loader)
    assert model.eval_feat4cls.shape == (R, spec.embed_dim) and model.eval_row_labels.cpu().tolist() == labels.tolist()
    r = _oracle_ragged(O, img, labels, dict(enumerate(JOB_SHOTS)), tok, _oracle_sd(O, "small"), pl)
    fw = _check_against_oracle(O, model, r, JOB_SHOTS, "ragged job")
    ok = _free_of_near_ties(r, C_JOB)
    # 21 of the 24 classes are out of reach of every near-tied argmax of the ORACLE on this job (a pure function of the seeds, counted on
    # the CPU before the GPU run; image seeds 2 / 4 / 12-15 x class-token seeds 1-8 were tried for the oracle ALONE to meet the floor: with
    # random weights the text rows of 24 classes lie close together).  They hold the fusion weights to the oracle's exactly; below 80 % the test fails
    assert ok.sum() >= 0.8 * C_JOB, f"only {int(ok.sum())} of {C_JOB} classes free of near-ties: this job no longer pins the fusion weights"
    np.testing.assert_allclose(fw.numpy()[ok], r["fusion_weight"].numpy()[ok], atol=1e-5)
    ragged_counts, ragged_tokens = model.xval_counts.cpu().clone(), model.visual_tokens.cpu().clone()
    # ---- the same items, filled: 16 rows per class, duplicates drawn with replacement
    filled = cli.layout_exemplars([(i, int(l)) for i, l in enumerate(labels)], CAP, seed=1)
    rows = torch.tensor([i for i, _ in filled])
    assert len(filled) == C_JOB * CAP and [l for _, l in filled] == np.repeat(np.arange(C_JOB), CAP).tolist()
    model.forward_prompt(ResidentEvalSet(img[rows], torch.arange(C_JOB), CAP, 2))
    assert model.eval_row_labels is None and model.eval_feat4cls.shape == (C_JOB, CAP, spec.embed_dim)
    filled_counts = model.xval_counts.cpu()
    assert filled_counts[:, 1].sum(-1).tolist() == [C_JOB * CAP] * 3 != [R] * 3          # a duplicate votes again
    assert model._n_label.cpu().tolist() == [CAP] * C_JOB != JOB_SHOTS
    full = torch.tensor([s == CAP for s in JOB_SHOTS])
    assert torch.equal(model.visual_tokens.cpu()[full], ragged_tokens[full])              # a full class is the same class either way
    assert not torch.equal(model.visual_tokens.cpu()[~full], ragged_tokens[~full])        # a filled one attends over its duplicates
    assert not torch.equal(filled_counts, ragged_counts)


def test_cli_ragged_shots_with_exemplar_list(tmp_path, O):
    """`--ragged-shots --exemplar-list` on a JPEG folder through the runner and its pipelined loader: 5 classes with 1 to 4 listed
    exemplars, NUM_SHOTS 4; the saved classifier rows against the oracle on the same decoded images, the file's keys, dtypes, shapes."""
    from PIL import Image
    from ovmr_amd import checkpoint, cli
    from ovmr_amd.tokenizer import BPETokenizer
    from test_hip_parity import _oracle_sd
    from test_next_rows_cpu import TRAINER_YAML, make_synthetic_bpe
    spec, shots = synth.SPECS["small"], [3, 1, 4, 2, 1]
    C, rng, root = len(shots), np.random.default_rng(3), tmp_path / "data"
    names = ["tench", "gold fish", "sea_horse", "yin yang", "tree frog"]
    for split, n in (("train", 5), ("val", 2)):
        for c in range(C):
            d = root / split / f"n{c:02d}"
            d.mkdir(parents=True)
            for i in range(n):
                base = np.full((70, 90, 3), 40 * c + 30, dtype=np.int32) + rng.integers(-25, 25, (70, 90, 3))
                Image.fromarray(base.clip(0, 255).astype(np.uint8)).save(d / f"{i}.jpg", quality=92)
    (root / "classnames.txt").write_text("".join(f"n{c:02d} {names[c]}\n" for c in range(C)))
    listed = [(str(root / "train" / f"n{c:02d}" / f"{i}.jpg"), c) for c in range(C) for i in range(shots[c])]
    (tmp_path / "exemplars.txt").write_text("".join(f"{p} {l}\n" for p, l in listed))
    bpe = str(tmp_path / "bpe.txt.gz")
    make_synthetic_bpe(bpe)
    torch.save({k: torch.from_numpy(v) for k, v in synth.clip_state_dict(spec, SEED, jitter=True).items()}, tmp_path / "clip.pt")
    pl_sd = {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, 2, SEED, True).items()}
    checkpoint.save_prompt_learner_state(pl_sd, str(tmp_path / "ckpt"), 30)
    Rs = spec.image_resolution
    (tmp_path / "trainer.yaml").write_text(TRAINER_YAML.replace("SIZE: (224, 224)", f"SIZE: ({Rs}, {Rs})").replace('NAME: "ViT-B/16"', 'NAME: ""')
                                           .replace("BATCH_SIZE: 256", "BATCH_SIZE: 6"))
    (tmp_path / "dataset.yaml").write_text('DATASET:\n  NAME: "ImageNet"\n')
    out = tmp_path / "out"
    res = cli.main(["--root", str(root), "--seed", "1", "--trainer", "MM_CLS_OP", "--dataset-config-file", str(tmp_path / "dataset.yaml"),
                    "--config-file", str(tmp_path / "trainer.yaml"), "--clip-weights", str(tmp_path / "clip.pt"), "--bpe-path", bpe,
                    "--model-dir", str(tmp_path / "ckpt"), "--load-epoch", "30", "--eval_mode", "fusion", "--eval_tau", "10", "--n_ctx", "2",
                    "--eval-only", "--output-dir", str(out), "--ragged-shots", "--exemplar-list", str(tmp_path / "exemplars.txt"),
                    "DATASET.NUM_SHOTS", "4", "DATASET.SUBSAMPLE_CLASSES", "all"])
    assert res["pipeline_exemplar"]["images"] == sum(shots) and res["pipeline_exemplar"]["batches"] == 3      # [3, 1] [4, 2] [1]: no filling
    assert res["classnames"] == names and 0.0 <= res["accuracy"] <= 100.0
    saved = torch.load(out / "mm_classifiers.pt", map_location="cpu")
    tokens = torch.load(out / "visual_tokens.pt", map_location="cpu")["visual_tokens"]
    D = spec.embed_dim
    assert sorted(saved) == ["fusion_weight", "mm_classifier", "text_classifier", "vision_classifier"]
    assert all(t.dtype == torch.float32 for t in saved.values()) and saved["mm_classifier"].shape == (C, D) and saved["fusion_weight"].shape == (C, 3)
    assert tokens.shape == (C, 2, D) and tokens.dtype == torch.float16
    tok = BPETokenizer(bpe).tokenize(["a " + n.replace("_", " ") + "." for n in names])
    img = torch.stack([cli.test_transform(Image.open(p), Rs) for p, _ in listed])
    r = _oracle_ragged(O, img, np.array([l for _, l in listed]), dict(enumerate(shots)), tok, _oracle_sd(O, "small"), pl_sd)
    for k, ref in (("mm_classifier", "mm"), ("vision_classifier", "v"), ("text_classifier", "t")):
        assert_cosine(saved[k].numpy(), r[ref].numpy(), COS_TOL, k)
    assert_cosine(tokens.float().numpy(), r["tokens"].float().numpy(), COS_TOL, "visual_tokens")
    np.testing.assert_allclose(saved["fusion_weight"].sum(-1).numpy(), 1.0, atol=1e-5)


@pytest.mark.timeout(600)
def test_two_process_ragged_job_bit_equal_to_one_process(tmp_path):
    """The ragged job as two gloo ranks sharing the GPU (class-sharded loaders: 12 + 12 classes, 84 rows each) against the one-process
    run: classes, counters, fusion weights and both files, bit for bit.  Each process under its own `timeout`."""
    import os
    import socket
    import subprocess
    import sys
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ragged_gpu_worker.py")

    def launch(world, result):
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        procs = [subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, worker, result],
                                  env=dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                                           HSA_ENABLE_IPC_MODE_LEGACY="0"),
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for rank in range(world)]
        outs = [p.communicate(timeout=300)[0] for p in procs]
        for p, o in zip(procs, outs):
            assert p.returncode == 0, o[-3000:]
        return torch.load(result)

    one = launch(1, str(tmp_path / "w1.pt"))
    two = launch(2, str(tmp_path / "w2.pt"))
    assert not one["sharded_path"] and two["sharded_path"] and one["local_rows"] == 168 and two["local_rows"] == 84
    assert one["classes"] == two["classes"] == list(range(24))
    for k in ("mm", "v", "t", "tokens", "counts", "w"):
        assert torch.equal(one[k], two[k]), f"{k} differs between one and two processes"
    assert sorted(one["files"]) == sorted(two["files"]) == ["mm_classifiers.pt", "visual_tokens.pt"]
    for f in one["files"]:
        for k, t in one["files"][f].items():
            assert t.dtype == two["files"][f][k].dtype and torch.equal(t, two["files"][f][k]), f"{f}: {k}"
