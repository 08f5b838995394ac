"""Ranked prediction above the kernel: Classification.process(topk) on the device, predict_topk / predict_topk_batches / load_classifiers of
the modules, and the runner's --predict mode.  The expected order is always the stable descending sort on the CPU (tests/test_hip_topk.py
holds the kernel to it).  Run with -m gpu on an MI355X."""
import csv
import os

import numpy as np
import pytest
import torch

from ovmr_amd import synth

pytestmark = pytest.mark.gpu

SEED = 11
NAN, INF = float("nan"), float("inf")
_MODELS = {}


def _stable(out, k):
    xf = out.float().cpu()
    idx = torch.sort(xf, dim=1, descending=True, stable=True)[1][:, :k]
    return xf.gather(1, idx), idx


def _clip(name="tiny", n_ctx=2):
    from ovmr_amd import modules
    if name not in _MODELS:
        spec = synth.SPECS[name]
        sd = {k: torch.from_numpy(v) for k, v in synth.clip_state_dict(spec, SEED, jitter=True).items()}
        _MODELS[name] = modules.CLIPModel(sd, spec)
    return _MODELS[name]


def _pl_state(name="tiny", n_ctx=2):
    return {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(synth.SPECS[name], n_ctx, SEED, True).items()}


# ----------------------------------------------------------------------------- evaluator
def test_device_evaluator_topk(tmp_path):
    """process(topk=3) over three batches on outputs with ties: accuracy / correct are the reference's literal formula
    (Dassl.pytorch/dassl/evaluation/evaluator.py:56-60) on the stable-sort indices; macro-F1 and both CSVs are those of a topk = 1 pass."""
    from ovmr_amd.evaluator import Classification
    B, C, k = 37, 70, 3
    g = torch.Generator().manual_seed(5)
    mo = torch.randint(0, 6, (B, C), generator=g).float()               # six values over seventy columns: ties in every row
    mo[0, :10] = torch.tensor([1, NAN, 3, 3, -0.0, 0.0, INF, NAN, -INF, 3])
    mo[1] = 2.0
    gt = torch.randint(0, C, (B,), generator=g)
    gt[0], gt[1] = 6, 3
    order = _stable(mo, k)[1]
    for r in range(2, 30, 3):                                           # labels at rank 0, k - 1 and k of their rows
        full = torch.sort(mo[r], descending=True, stable=True)[1]
        gt[r] = full[(0, k - 1, k)[(r // 3) % 3]]
    matches = (order == (gt.unsqueeze(1).repeat(1, k))).float().sum(dim=-1)                      # :58
    correct = int(matches.sum().item())
    assert 0 < correct < B
    cuts = [0, 13, 13, 30, B]

    def run(topk, sub, dtype=torch.float32):
        ev = Classification(C, device="cuda")
        dev, lab = mo.to(dtype).cuda(), gt.cuda()
        for a, b in zip(cuts[:-1], cuts[1:]):
            ev.process(dev[a:b], lab[a:b], **({"topk": topk} if topk != 1 else {}))
        return ev, ev.evaluate(str(tmp_path / sub))

    ev3, res3 = run(k, "k3")
    ev1, res1 = run(1, "k1")
    assert res3["accuracy"] == pytest.approx(100.0 * correct / B) and res3["error_rate"] == pytest.approx(100.0 - res3["accuracy"])
    assert int(ev3._hits.cpu()) == correct
    assert res1["accuracy"] == pytest.approx(100.0 * float((order[:, 0] == gt).float().mean())) and res1["accuracy"] < res3["accuracy"]
    assert res3["macro_f1"] == res1["macro_f1"]
    for name in ("acc_per_class.csv", "f1_per_class.csv"):
        assert (tmp_path / "k3" / name).read_bytes() == (tmp_path / "k1" / name).read_bytes()
    assert all(torch.equal(a, b) for a, b in zip(ev3.counts(), ev1.counts()))
    _, res16 = run(k, "k3h", torch.float16)                             # the same small integers in fp16
    assert res16["accuracy"] == res3["accuracy"]
    with pytest.raises(ValueError, match="one topk"):
        ev3.process(mo.cuda(), gt.cuda(), topk=2)
    with pytest.raises(ValueError, match="one topk"):
        ev1.process(mo.cuda(), gt.cuda(), topk=3)
    host = Classification(C, device="cpu")                              # the host path: the same figure
    host.process(mo, gt, topk=k)
    assert int(host._hits) == correct


# ----------------------------------------------------------------------------- modules
def _tiny_job(golden, out_dir):
    from ovmr_amd import modules
    g = golden("tiny")
    spec = synth.SPECS["tiny"]
    S, cpb = int(g["meta_shots"]), int(g["meta_classes_per_batch"])
    labels = g["l2_eval_labels"]
    img = synth.images(len(labels), spec.image_resolution, seed=1234, class_ids=labels, class_strength=0.6)
    loader = [{"img": torch.from_numpy(img[s:s + cpb * S]), "label": torch.from_numpy(labels[s:s + cpb * S])} for s in range(0, len(labels), cpb * S)]

    def make(sub):
        cfg = modules.make_cfg(n_ctx=2, num_shots=S, eval_tau=float(g["meta_tau"]), output_dir=str(out_dir / sub))
        return modules.CustomCLIP(cfg, torch.from_numpy(g["l2_tokenized_prompts"]), _clip(), prompt_learner_state=_pl_state(), reserve=(64, 64, 256))

    batches = [torch.from_numpy(synth.images(n, spec.image_resolution, seed=700 + n)) for n in (5, 4, 3)]
    return g, make, loader, batches


def _check_ranked(pair, out, k):
    values, indices = pair
    assert values.dtype == torch.float32 and indices.dtype == torch.int64 and values.shape == indices.shape == (out.shape[0], k)
    want_v, want_i = _stable(out, k)
    assert torch.equal(indices.cpu(), want_i) and torch.equal(values.cpu(), want_v)


def test_custom_clip_predict_topk_and_load_classifiers(golden, tmp_path):
    g, make, loader, batches = _tiny_job(golden, tmp_path)
    m = make("gen")
    C = len(m.tokenized_prompts)
    k = min(5, C)
    first = m.predict_topk(batches[0], k, eval_set_loader=loader)       # the first call generates the classifiers, as forward does
    outs = [m(b) for b in batches]
    assert outs[0].shape == (5, C) and outs[0].dtype == torch.float32
    _check_ranked(first, outs[0], k)
    per_batch = [m.predict_topk(b, k) for b in batches]
    for pair, out in zip(per_batch, outs):
        _check_ranked(pair, out, k)
    got = list(m.predict_topk_batches(iter(batches), k))
    assert len(got) == 3
    for (v, i), (pv, pi) in zip(got, per_batch):
        assert torch.equal(v, pv) and torch.equal(i, pi)
    assert all(torch.equal(a, b) for a, b in zip(m.forward_batches(iter(batches)), outs))        # the [B, C] outputs are untouched
    with pytest.raises(Exception):
        m.predict_topk(batches[0], C + 1)
    # load_classifiers: a second model reads the written file and computes the same bits without generating anything
    m.wait_files()
    path = tmp_path / "gen" / "mm_classifiers.pt"
    m2 = make("loaded")
    with pytest.raises(NotImplementedError):
        m2(batches[0])
    m2.load_classifiers(str(path))
    for a, b in ((m2.mm_classifier, m.mm_classifier), (m2.visual_classifer, m.visual_classifer), (m2.zero_shot_classifier, m.zero_shot_classifier),
                 (m2.fusion_weight, m.fusion_weight)):
        assert a.dtype == b.dtype and a.device == b.device and torch.equal(a, b)
    assert m2.prompt_learner.zero_shot_classifier is m2.zero_shot_classifier
    for b, out in zip(batches, outs):
        assert torch.equal(m2(b), out)
    for (v, i), (pv, pi) in zip(m2.predict_topk_batches(iter(batches), k), per_batch):          # both handles read the loaded state
        assert torch.equal(v, pv) and torch.equal(i, pi)
    assert not (tmp_path / "loaded").exists()                           # nothing generated, nothing written
    # a file for another class count, or another width, is refused
    saved = torch.load(path, map_location="cpu")
    wrong = {k_: torch.cat([v, v[:1]]) for k_, v in saved.items()}
    torch.save(wrong, tmp_path / "wrong_c.pt")
    with pytest.raises(ValueError, match=f"{C} classes"):
        make("x").load_classifiers(str(tmp_path / "wrong_c.pt"))
    narrow = {k_: (v if k_ == "fusion_weight" else v[:, :-1].contiguous()) for k_, v in saved.items()}
    torch.save(narrow, tmp_path / "wrong_d.pt")
    with pytest.raises(ValueError, match="width"):
        make("x").load_classifiers(str(tmp_path / "wrong_d.pt"))
    torch.save({"mm_classifier": saved["mm_classifier"]}, tmp_path / "partial.pt")
    with pytest.raises(ValueError, match="mm_classifiers.pt"):
        make("x").load_classifiers(str(tmp_path / "partial.pt"))


def test_zeroshot_predict_topk(golden, tmp_path):
    from ovmr_amd import modules
    g, _, _, batches = _tiny_job(golden, tmp_path)
    m = modules.ZeroshotCLIP(_clip(), torch.from_numpy(g["l2_tokenized_prompts"]), reserve=(64, 64, 256))
    C = m.text_features.shape[0]
    k = min(5, C)
    outs = [m.model_inference(b) for b in batches]
    assert outs[0].dtype == torch.float16 and outs[0].shape == (5, C)
    per_batch = [m.predict_topk(b, k) for b in batches]
    for pair, out in zip(per_batch, outs):
        _check_ranked(pair, out, k)
    got = list(m.predict_topk_batches(iter(batches), k))
    assert len(got) == 3
    for (v, i), (pv, pi) in zip(got, per_batch):
        assert torch.equal(v, pv) and torch.equal(i, pi)
    assert all(torch.equal(a, b) for a, b in zip(m.inference_batches(iter(batches)), outs))


# ----------------------------------------------------------------------------- runner
NAMES = ["accordion", "sea_horse", "stop_sign", "yin_yang"]


def _dataset(tmp_path, golden, spec):
    """The class folders of the runner tests plus a folder of unlabelled JPEGs, the BPE fixture, the CLIP weights."""
    from PIL import Image
    from test_zeroshot_cpu import zsclip_bpe
    rng = np.random.default_rng(3)
    root = tmp_path / "data"
    for c in range(len(NAMES)):
        d = root / "train" / f"n{c:02d}"
        d.mkdir(parents=True)
        for i in range(2):
            base = np.full((70, 90, 3), 40 * c + 30, dtype=np.int32) + rng.integers(-25, 25, (70, 90, 3))
            Image.fromarray(base.clip(0, 255).astype(np.uint8)).save(d / f"{i}.png")
    (root / "classnames.txt").write_text("".join(f"n{c:02d} {n}\n" for c, n in enumerate(NAMES)))
    pics = tmp_path / "pics"
    for i, sub in enumerate(["b", "a/deep", "b", "a", "c", "a/deep", "b"]):
        (pics / sub).mkdir(parents=True, exist_ok=True)
        base = np.full((50 + 3 * i, 80 - 2 * i, 3), 35 * i + 20, dtype=np.int32) + rng.integers(-20, 20, (50 + 3 * i, 80 - 2 * i, 3))
        Image.fromarray(base.clip(0, 255).astype(np.uint8)).save(pics / sub / f"img{i}.jpg", quality=92)
    (pics / "notes.txt").write_text("not an image")
    bpe = str(tmp_path / "bpe.txt.gz")
    zsclip_bpe(bpe, golden)
    clip_sd = {k: torch.from_numpy(v) for k, v in synth.clip_state_dict(spec, SEED, jitter=True).items()}
    torch.save(clip_sd, tmp_path / "clip.pt")
    return root, pics, bpe, clip_sd


def _read_csv(path):
    text = open(path).read()
    rows = list(csv.reader(text.splitlines()))
    assert rows[0] == ["image", "rank", "label", "classname", "score"]
    return rows[1:]


def _check_csv(res, path, images, k, names):
    rows = _read_csv(path)
    assert len(rows) == len(images) * k
    assert [r[0] for r in rows] == [p for p in images for _ in range(k)] and [int(r[1]) for r in rows] == list(range(k)) * len(images)
    preds = res["predictions"]
    assert [p for p, _ in preds] == images and all(len(r) == k for _, r in preds)
    flat = [x for _, r in preds for x in r]
    assert [int(r[2]) for r in rows] == [x[0] for x in flat] and [r[3] for r in rows] == [x[1] for x in flat] == [names[x[0]] for x in flat]
    assert [float(r[4]) for r in rows] == [x[2] for x in flat]                                   # repr(float) parses back exactly
    assert all(r[4] == repr(x[2]) for r, x in zip(rows, flat))
    return preds


def _decoded_batches(images, R, B):
    from PIL import Image
    from ovmr_amd import cli
    imgs = torch.stack([cli.test_transform(Image.open(p), R, interpolation="bilinear", mean=None) for p in images])
    return [imgs[s:s + B] for s in range(0, len(images), B)]


def test_runner_predict_zeroshot(golden, tmp_path, capsys):
    from ovmr_amd import cli, modules
    from ovmr_amd.tokenizer import BPETokenizer
    spec, B, k = synth.SPECS["tiny"], 3, 3
    R = spec.image_resolution
    root, pics, bpe, clip_sd = _dataset(tmp_path, golden, spec)
    out = tmp_path / "out"
    argv = ["--root", str(root), "--seed", "1", "--trainer", "ZeroshotCLIP", "--eval-only", "--clip-weights", str(tmp_path / "clip.pt"),
            "--bpe-path", bpe, "--output-dir", str(out), "--workers", "2", "--predict", str(pics), "--topk", str(k),
            "--test-split", "no_such_split",                           # the labelled test split is not listed
            "DATASET.NAME", "Caltech101", "INPUT.SIZE", f"({R}, {R})", "DATALOADER.TEST.BATCH_SIZE", str(B)]
    res = cli.main(argv)
    images = sorted(str(p) for p in pics.rglob("*.jpg"))
    assert len(images) == 7 and res["classnames"] == NAMES and res["pipeline_predict"]["images"] == 7
    assert sorted(p.name for p in out.iterdir()) == ["predictions.csv"]
    preds = _check_csv(res, out / "predictions.csv", images, k, NAMES)
    model = modules.ZeroshotCLIP.from_classnames(modules.CLIPModel(clip_sd, spec), NAMES, "Caltech101", BPETokenizer(bpe))
    logits = torch.cat([model.model_inference(b) for b in _decoded_batches(images, R, B)])
    assert [r[0][0] for _, r in preds] == logits.float().argmax(1).cpu().tolist()
    # a list file: file order, the default k = 5 is refused for four classes, k = 4 = C runs
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join([images[4], images[0], images[4]]) + "\n")
    with pytest.raises(SystemExit, match="--topk 5.*4 classes"):
        cli.main([a if a != str(pics) else str(lst) for a in argv[:argv.index("--topk")]] + argv[argv.index("--topk") + 2:])
    argv4 = [a if a != str(pics) else str(lst) for a in argv]
    argv4[argv4.index("--topk") + 1] = "4"
    res4 = cli.main(argv4)
    preds4 = _check_csv(res4, out / "predictions.csv", [images[4], images[0], images[4]], 4, NAMES)
    assert preds4[0][1] == preds4[2][1] and preds4[0][1][:k] == preds[4][1] and preds4[1][1][:k] == preds[0][1]
    assert all(sorted(x[0] for x in r) == [0, 1, 2, 3] for _, r in preds4)


def test_runner_predict_mm_cls_op_and_classifiers_file(golden, tmp_path):
    from ovmr_amd import checkpoint, cli, config, modules
    from ovmr_amd.tokenizer import BPETokenizer
    spec, B, k, S = synth.SPECS["tiny"], 4, 2, 2
    R = spec.image_resolution
    root, pics, bpe, clip_sd = _dataset(tmp_path, golden, spec)
    checkpoint.save_prompt_learner_state(_pl_state(), str(tmp_path / "ckpt"), 30)
    out = tmp_path / "out"
    common = ["--root", str(root), "--seed", "1", "--trainer", "MM_CLS_OP", "--eval-only", "--clip-weights", str(tmp_path / "clip.pt"),
              "--bpe-path", bpe, "--model-dir", str(tmp_path / "ckpt"), "--load-epoch", "30", "--eval_mode", "fusion", "--eval_tau", "10",
              "--n_ctx", "2", "--workers", "2", "--predict", str(pics), "--topk", str(k)]
    opts = ["DATASET.NAME", "ImageNet", "INPUT.SIZE", f"({R}, {R})", "DATALOADER.TEST.BATCH_SIZE", str(B), "DATASET.NUM_SHOTS", str(S)]
    res = cli.main(common + ["--output-dir", str(out)] + opts)
    images = sorted(str(p) for p in pics.rglob("*.jpg"))
    assert res["pipeline_exemplar"]["images"] == len(NAMES) * S and res["pipeline_predict"]["images"] == 7
    assert sorted(p.name for p in out.iterdir()) == ["mm_classifiers.pt", "predictions.csv", "visual_tokens.pt"]      # both model files as today
    preds = _check_csv(res, out / "predictions.csv", images, k, NAMES)
    # the module's own outputs on the same decoded images, from the written classifiers
    cfg = config.setup_cfg(cli.parse(common + ["--output-dir", str(tmp_path / "unused")] + opts))
    tk = BPETokenizer(bpe)
    m = modules.CustomCLIP(cfg, NAMES, modules.CLIPModel(clip_sd, spec), tokenizer=tk, prompt_learner_state=_pl_state(), reserve=(B, 256, 1024))
    m.load_classifiers(str(out / "mm_classifiers.pt"))
    probs = torch.cat([m(b) for b in _decoded_batches(images, R, B)])
    assert [r[0][0] for _, r in preds] == probs.argmax(1).cpu().tolist()
    # the same job from the written classifiers: byte-equal predictions, no exemplar decoded, no model file written
    out2 = tmp_path / "out2"
    first = (out / "predictions.csv").read_bytes()
    res2 = cli.main(common + ["--output-dir", str(out2), "--classifiers", str(out / "mm_classifiers.pt")] + opts)
    assert "pipeline_exemplar" not in res2 and res2["pipeline_predict"]["images"] == 7
    assert sorted(p.name for p in out2.iterdir()) == ["predictions.csv"]
    assert (out2 / "predictions.csv").read_bytes() == first and res2["predictions"] == res["predictions"]
    # ... also into a directory that already holds results (no "results exist" early exit), and without DATASET.NUM_SHOTS
    res3 = cli.main(common + ["--output-dir", str(out), "--classifiers", str(out / "mm_classifiers.pt")] + opts[:-2])
    assert res3["predictions"] == res["predictions"] and (out / "predictions.csv").read_bytes() == first
