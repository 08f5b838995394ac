"""Zero-shot trainers on the HIP path (trainers/zsclip.py): ovmr_encode_text_ensemble (csrc/text_ensemble.hip) against the reference's fp16
arithmetic on the GPU, its chunking and calling rules, ZeroshotCLIP / ZeroshotCLIP2 against the real reference (tests/golden/zsclip.npz,
tests/golden/gen_zsclip.py), and the runner / trainer end to end.  Needs an MI355X: `pytest -m gpu`."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import COS_TOL, assert_cosine, cosine_rows
from ovmr_amd import synth

pytestmark = pytest.mark.gpu
SEED = 11
_ENGINES = {}


def _engine(name, reserve=(64, 64, 256)):
    """An Engine with the seeded synthetic CLIP weights of `name`, finalised with `reserve` (cached per (name, reserve))."""
    from ovmr_amd.runtime import Engine
    key = (name, tuple(reserve))
    if key not in _ENGINES:
        spec = synth.SPECS[name]
        e = Engine(spec, 2)
        e.load_state_dict({k: torch.from_numpy(v) for k, v in synth.clip_state_dict(spec, SEED, jitter=True).items()},
                          {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, 2, SEED, True).items()})
        e.finalize(*reserve)
        _ENGINES[key] = e
    return _ENGINES[key]


def _ids(T, C, seed, lo=3, hi=14, context=77):
    """[T, C, context] prompts: SOT, a template-dependent number of random tokens, EOT, zero padding (EOT = the largest id)."""
    rng = np.random.default_rng(seed)
    ids = np.zeros((T, C, context), dtype=np.int64)
    for t in range(T):
        base = lo + (5 * t) % (hi - lo)
        for c in range(C):
            n = base + int(rng.integers(0, 4))
            ids[t, c, 0] = synth.SOT_ID
            ids[t, c, 1:1 + n] = rng.integers(1, synth.SOT_ID, n)
            ids[t, c, 1 + n] = synth.EOT_ID
    return torch.from_numpy(ids)


def _seq_lens(ids):
    return (ids.argmax(-1).amax(1) + 1).tolist()


def _reference_ensemble(raw):
    """trainers/zsclip.py:88-96 in torch, fp16 on the GPU; raw: [T, C, E] fp16 features of encode_text."""
    mean_text_features = 0
    for t in range(raw.shape[0]):
        text_features = raw[t]
        text_features = text_features / text_features.norm(dim=-1, keepdim=True)
        mean_text_features = mean_text_features + text_features
    mean_text_features = mean_text_features / raw.shape[0]
    return mean_text_features / mean_text_features.norm(dim=-1, keepdim=True)


def _ulps(a, b):
    """Distance in fp16 steps between two fp16 tensors of finite values."""
    def ordered(x):
        i = x.contiguous().view(torch.int16).int()
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (ordered(a) - ordered(b)).abs()


def _order_sensitive(x):
    """[..., E] fp16 rows whose h(||x||) may depend on the fp32 summation order of the squares: the exact norm lies within 1e-5 (relative,
    some 20 times the typical fp32 summation error) of a rounding boundary between two fp16 values."""
    x = x.double().cpu().numpy()
    n = np.sqrt((x * x).sum(-1))
    h = n.astype(np.float16)
    up, dn = np.nextafter(h, np.float16(np.inf)), np.nextafter(h, np.float16(-np.inf))
    d = np.minimum(np.abs(n - (h.astype(np.float64) + up) / 2), np.abs(n - (h.astype(np.float64) + dn) / 2))
    return d < 1e-5 * n


@pytest.mark.parametrize("name", ["tiny", "small", "ViT-B/16", "head768"])
@pytest.mark.parametrize("T", [1, 7, 8, 13])
def test_ensemble_kernel_matches_the_reference_arithmetic(name, T):
    """The ensemble launch against the torch fp16 statement of zsclip.py:88-96 on the GPU, fed with the raw per-template rows of
    encode_text_groups (the same T groups in one pass: the entry point's own tower pass, bit for bit).  >= 99 % of the elements
    bit-equal and every element within one fp16 step, on every class whose T + 1 norms are decided: a class where one of them lies so close
    to an fp16 rounding boundary that the fp32 summation order of its squares (the only freedom) decides it is held to 1 - cos <= 1e-6 only
    -- one fp16 step of a norm moves a whole template row (all E elements of the class), and where the templates nearly cancel that is
    several steps of the sum.  E = 128, 256, 512, 768."""
    e = _engine(name, (64, 512, 256))                     # the workspace takes all T groups in one pass, here and in the entry point
    C = 64
    ids = _ids(T, C, seed=T)
    sl = _seq_lens(ids)
    raw = torch.stack(e.encode_text_groups([dict(ids=ids[t], seq_len=sl[t], normalize=0) for t in range(T)]))
    got = e.encode_text_ensemble(ids)
    want = _reference_ensemble(raw)
    torch.cuda.synchronize()
    assert got.shape == (C, e.spec.embed_dim) and got.dtype == torch.float16
    assert bool(torch.isfinite(got.float()).all())
    d = _ulps(got, want).cpu().numpy()
    mean = raw[0] / raw[0].norm(dim=-1, keepdim=True)
    for t in range(1, T):
        mean = mean + raw[t] / raw[t].norm(dim=-1, keepdim=True)
    loose = _order_sensitive(raw).any(0) | _order_sensitive(mean / T)
    assert (~loose).sum() >= C // 4, f"{name} T={T}: {loose.sum()} of {C} classes near a rounding boundary"
    assert d[~loose].max() <= 1, f"{name} T={T}: {int(d[~loose].max())} fp16 steps on a class whose norms are decided"
    assert float((d[~loose] == 0).mean()) >= 0.99, f"{name} T={T}: only {float((d[~loose] == 0).mean()):.4f} bit-equal"
    c = cosine_rows(got.float().cpu().numpy(), want.float().cpu().numpy())
    assert (1.0 - c).max() <= 1e-6, f"{name} T={T}: 1 - cos {(1.0 - c).max():.2e}"
    # device ids (no host-side lengths): the full context -- the same classifier up to the GEMM choice of the longer rows
    full = e.encode_text_ensemble(ids.cuda())
    assert_cosine(full.float().cpu().numpy(), got.float().cpu().numpy(), 1e-5, "full context vs exact lengths")


def test_chunking_streams_and_graph_replay():
    """C = 3000 classes x T = 8 templates on a handle finalised for 32 prompts: several chunks.  Against a handle that
    takes all classes in one pass (the row count may pick other GEMM kernels: 1 - cos <= 1e-6); bit-identical over two runs, a second
    stream and a graph replay."""
    T, C = 8, 3000
    ids = _ids(T, C, seed=5)
    sl = _seq_lens(ids)
    small = _engine("small", (1, 32, 8))
    big = _engine("small", (1, 4500, 256))
    assert C * sum(sl) < 4500 * 77                        # one pass on the big handle; the small one's workspace (the 200 MB floor of
                                                          # ovmr_finalize) holds some 400 classes of these 8 templates: several chunks
    a = small.encode_text_ensemble(ids)
    b = small.encode_text_ensemble(ids)
    one = big.encode_text_ensemble(ids)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    c = cosine_rows(a.float().cpu().numpy(), one.float().cpu().numpy())
    assert (1.0 - c).max() <= 1e-6, f"chunked vs one pass: 1 - cos {(1.0 - c).max():.2e}"
    dev = ids.cuda()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        s = small.encode_text_ensemble(dev, seq_lens=sl)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    assert torch.equal(s, a)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g = small.encode_text_ensemble(dev, seq_lens=sl)
    g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g, a)
    # a shorter vocabulary through the same handle, then the captured graph again: the replay does not depend on the call in between
    small.encode_text_ensemble(_ids(T, 5, seed=9))
    g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g, a)


def test_argument_errors():
    from ovmr_amd import runtime
    e = _engine("tiny")
    lib = e.lib
    ids = _ids(3, 4, seed=1).cuda()
    out = torch.empty(4, e.spec.embed_dim, dtype=torch.float16, device="cuda")
    s = runtime._stream()
    lens = lambda *v: (ctypes.c_int32 * len(v))(*v)                    # noqa: E731
    P = runtime._ptr
    assert lib.ovmr_encode_text_ensemble(None, P(ids), 3, 4, None, P(out), s) == -1
    assert lib.ovmr_encode_text_ensemble(e.h, None, 3, 4, None, P(out), s) == -1
    assert lib.ovmr_encode_text_ensemble(e.h, P(ids), 3, 4, None, None, s) == -1
    assert lib.ovmr_encode_text_ensemble(e.h, P(ids), 0, 4, None, P(out), s) == -1
    assert lib.ovmr_encode_text_ensemble(e.h, P(ids), 3, -1, None, P(out), s) == -1
    assert lib.ovmr_encode_text_ensemble(e.h, P(ids), 3, 4, lens(20, 0, 20), P(out), s) == -1
    assert lib.ovmr_encode_text_ensemble(e.h, P(ids), 3, 4, lens(20, 78, 20), P(out), s) == -1
    assert lib.ovmr_encode_text_ensemble(e.h, None, 3, 0, None, None, s) == 0          # C == 0: nothing to do
    assert lib.ovmr_encode_text_ensemble(e.h, P(ids), 3, 4, lens(20, 20, 20), P(out), s) == 0
    # one class's T prompts larger than the workspace: refused, nothing launched
    many = _ids(2000, 1, seed=2).cuda()                                 # 2000 x 77 token rows of one class: > the workspace
    out2 = torch.empty(1, e.spec.embed_dim, dtype=torch.float16, device="cuda")
    assert lib.ovmr_encode_text_ensemble(e.h, P(many), 2000, 1, None, P(out2), s) == -2
    assert b"workspace" in lib.ovmr_last_error(e.h)
    # host-side checks of the binding
    host = _ids(3, 4, seed=1)
    with pytest.raises(ValueError, match="EOT"):
        e.encode_text_ensemble(host, seq_lens=[2, 2, 2])
    with pytest.raises(ValueError, match="templates"):
        e.encode_text_ensemble(host, seq_lens=[20, 20])
    assert e.encode_text_ensemble(host[:, :0]).shape == (0, e.spec.embed_dim)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- against the reference (tests/golden/zsclip.npz)
_CLIP = {}


def _vitb16():
    from ovmr_amd import modules
    if "m" not in _CLIP:
        spec = synth.SPECS["ViT-B/16"]
        _CLIP["m"] = modules.CLIPModel({k: torch.from_numpy(v) for k, v in synth.clip_state_dict(spec, SEED, jitter=True).items()}, spec)
    return _CLIP["m"]


def _tokenizer(golden, tmp_path):
    from ovmr_amd.tokenizer import BPETokenizer
    from test_zeroshot_cpu import zsclip_bpe
    zsclip_bpe(str(tmp_path / "bpe.txt.gz"), golden)
    return BPETokenizer(str(tmp_path / "bpe.txt.gz"))


def _check_logits(got, ref, what):
    assert_cosine(got, ref, COS_TOL, what)
    top2 = np.sort(ref, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 0.05
    assert clear.sum() >= len(ref) // 2, f"{what}: only {clear.sum()} rows with a clear reference argmax"
    assert np.array_equal(got.argmax(1)[clear], ref.argmax(1)[clear]), f"{what}: argmax differs on a clear row"


def test_zeroshot_clip2_vs_golden(golden, capsys):
    from ovmr_amd import modules
    g = golden("zsclip")
    cm = _vitb16()
    img = torch.from_numpy(synth.images(int(g["zs_meta_n_img"]), 224, seed=int(g["zs_meta_img_seed"])))
    ids = torch.from_numpy(g["zs_token_ids"])
    report = {}
    for key, sub in (("zsclip2", ids), ("zsclip2_imagenet", ids[:7])):
        m = modules.ZeroshotCLIP2(cm, sub)
        tf = m.text_features.float().cpu().numpy()
        for tag in ("fp16", "fp32"):
            assert_cosine(tf, g[f"{key}_{tag}_text_features"], COS_TOL, f"{key} text features vs reference {tag}")
            report[f"{key} {tag}"] = f"{(1 - cosine_rows(tf, g[f'{key}_{tag}_text_features'])).max():.2e}"
        if key == "zsclip2":
            logits = m.model_inference(img).float().cpu().numpy()
            for tag in ("fp16", "fp32"):
                _check_logits(logits, g[f"zsclip2_{tag}_logits"], f"ZeroshotCLIP2 logits vs reference {tag}")
    assert "Prompt ensembling (n=8)" in capsys.readouterr().out
    with capsys.disabled():
        print("\n1 - cos of the ensembled text features vs the reference (max over 10 classes):", report)


def test_from_classnames_vs_golden(golden, tmp_path, capsys):
    from ovmr_amd import modules
    g = golden("zsclip")
    tk = _tokenizer(golden, tmp_path)
    cm = _vitb16()
    names = [str(c) for c in g["zs_classnames"]]
    img = torch.from_numpy(synth.images(int(g["zs_meta_n_img"]), 224, seed=int(g["zs_meta_img_seed"])))
    one = modules.ZeroshotCLIP.from_classnames(cm, names, "Caltech101", tk)
    out = capsys.readouterr().out
    assert "Prompts: ['a photo of a accordion.'" in out and "'a photo of a sea horse.'" in out
    assert torch.equal(one.tokenized_prompts, torch.from_numpy(g["zs_token_ids"][7]))
    tf = one.text_features.float().cpu().numpy()
    logits = one.model_inference(img).float().cpu().numpy()
    for tag in ("fp16", "fp32"):
        assert_cosine(tf, g[f"zsclip_{tag}_text_features"], COS_TOL, f"ZeroshotCLIP text features vs reference {tag}")
        _check_logits(logits, g[f"zsclip_{tag}_logits"], f"ZeroshotCLIP logits vs reference {tag}")
    # the existing constructor on the fixture's ids: the same classifier
    assert torch.equal(modules.ZeroshotCLIP(cm, torch.from_numpy(g["zs_token_ids"][7])).text_features, one.text_features)
    two = modules.ZeroshotCLIP2.from_classnames(cm, names, "Caltech101", tk)
    assert torch.equal(two.tokenized_prompts, torch.from_numpy(g["zs_token_ids"]))
    assert torch.equal(two.text_features, modules.ZeroshotCLIP2(cm, torch.from_numpy(g["zs_token_ids"])).text_features)
    assert modules.ZeroshotCLIP2.from_classnames(cm, names, "ImageNet", tk).tokenized_prompts.shape == (7, 10, 77)
    with pytest.raises(KeyError, match="known datasets"):
        modules.ZeroshotCLIP2.from_classnames(cm, names, "ImageNet21kP", tk)


# ----------------------------------------------------------------------------- end to end
def _folder_dataset(tmp_path, names, n_val=3):
    from PIL import Image
    rng = np.random.default_rng(3)
    root = tmp_path / "data"
    for split, n in (("train", 2), ("val", n_val)):
        for c in range(len(names)):
            d = root / split / f"n{c:02d}"
            d.mkdir(parents=True)
            for i in range(n):
                base = np.full((70, 90, 3), 40 * c + 30, dtype=np.int32) + rng.integers(-25, 25, (70, 90, 3))
                Image.fromarray(base.clip(0, 255).astype(np.uint8)).save(d / f"{i}.png")
    (root / "classnames.txt").write_text("".join(f"n{c:02d} {n}\n" for c, n in enumerate(names)))
    return root


def _expected(model, batches, labels, C):
    """Accuracy, macro-F1 and both per-class CSVs (Dassl's Classification evaluator, evaluator.py:69-138) through sklearn on the
    predictions of ZeroshotCLIP2.model_inference over the given decoded batches."""
    from sklearn.metrics import f1_score
    pred = np.concatenate([model.model_inference(b).float().argmax(1).cpu().numpy() for b in batches])
    y = np.asarray(labels)
    present = np.unique(y)
    acc = 100.0 * float((pred == y).mean())
    f1 = 100.0 * f1_score(y, pred, average="macro", labels=present)
    per_f1 = list(100.0 * f1_score(y, pred, average=None, labels=present))
    per_acc = {str(c): 100.0 * float((pred[y == c] == c).mean()) for c in present}
    return acc, f1, per_acc, per_f1


def _check_outputs(res, out_dir, want):
    acc, f1, per_acc, per_f1 = want
    assert res["accuracy"] == pytest.approx(acc) and res["macro_f1"] == pytest.approx(f1)
    assert res["error_rate"] == pytest.approx(100.0 - acc)
    acc_rows = open(out_dir / "acc_per_class.csv").read().strip().split("\n")
    assert acc_rows[0] == "Label,Acc" and {x.split(",")[0]: float(x.split(",")[1]) for x in acc_rows[1:]} == pytest.approx(per_acc)
    f1_rows = open(out_dir / "f1_per_class.csv").read().strip().split("\n")
    assert f1_rows[0] == "Label,F1" and [float(x.split(",")[1]) for x in f1_rows[1:]] == pytest.approx(per_f1)


def test_cli_and_trainer_end_to_end(golden, tmp_path, capsys):
    """`--eval-only --trainer ZeroshotCLIP2` on a PNG folder data set (built as the MM_CLS_OP runner test builds one), and the same job
    through trainer.build_trainer(cfg, dm).test(): accuracy, macro-F1 and both CSVs equal sklearn's figures on the predictions of
    ZeroshotCLIP2.model_inference over the same decoded batches; no model file is written."""
    from PIL import Image
    from ovmr_amd import cli, config, modules, trainer
    names = ["accordion", "sea_horse", "stop_sign", "yin_yang"]
    spec, C, B = synth.SPECS["small"], 4, 5
    R = spec.image_resolution
    root = _folder_dataset(tmp_path, names)
    bpe = str(tmp_path / "bpe.txt.gz")
    from test_zeroshot_cpu import zsclip_bpe
    zsclip_bpe(bpe, golden)
    clip_sd = {k: torch.from_numpy(v) for k, v in synth.clip_state_dict(spec, SEED, jitter=True).items()}
    torch.save(clip_sd, tmp_path / "clip.pt")
    out = tmp_path / "out"
    argv = ["--root", str(root), "--seed", "1", "--trainer", "ZeroshotCLIP2", "--eval-only", "--clip-weights", str(tmp_path / "clip.pt"),
            "--bpe-path", bpe, "--output-dir", str(out), "--workers", "2",
            "DATASET.NAME", "Caltech101", "INPUT.SIZE", f"({R}, {R})", "DATALOADER.TEST.BATCH_SIZE", str(B)]
    res = cli.main(argv)
    printed = capsys.readouterr().out
    assert "Prompt ensembling (n=8)" in printed and "* accuracy:" in printed
    assert res["classnames"] == names and res["pipeline_test"]["images"] == 3 * C
    assert sorted(p.name for p in out.iterdir()) == ["acc_per_class.csv", "f1_per_class.csv"]      # no model files
    # the expected figures: the same test items decoded by the PIL transform, the same batches, ZeroshotCLIP2.model_inference
    from ovmr_amd.tokenizer import BPETokenizer
    tk = BPETokenizer(bpe)
    cm = modules.CLIPModel(clip_sd, spec)
    model = modules.ZeroshotCLIP2.from_classnames(cm, names, "Caltech101", tk)
    _, items = cli.list_split(str(root), "val")
    imgs = torch.stack([cli.test_transform(Image.open(p), R, interpolation="bilinear", mean=None) for p, _ in items])
    batches = [imgs[s:s + B] for s in range(0, len(items), B)]
    want = _expected(model, batches, [l for _, l in items], C)
    _check_outputs(res, out, want)
    assert cli.main(argv) is not None                                  # no "results exist, skip" for the zero-shot trainers
    # the trainer path: Dassl's build_trainer(cfg) -> test()
    cfg = config.setup_cfg(cli.parse(argv))
    cfg.OUTPUT_DIR = str(tmp_path / "out_trainer")
    from types import SimpleNamespace
    loader = cli.FolderLoader(items, B, R, interpolation="bilinear", mean=None, std=None)
    dm = SimpleNamespace(dataset=SimpleNamespace(classnames=names), test_loader=loader, val_loader=None)
    tr = trainer.build_trainer(cfg, dm, clip_weights=clip_sd, tokenizer=tk)
    assert isinstance(tr, trainer.ZeroshotCLIP2)
    tr.load_model("")
    acc = tr.test()
    _check_outputs(tr.evaluator.evaluate(None), tmp_path / "out_trainer", want)
    assert acc == pytest.approx(want[0])
    assert torch.equal(tr.text_features, model.text_features)
    b = next(iter(loader))
    x, y = tr.parse_batch_test(b)
    assert torch.equal(tr.model_inference(x), model.model_inference(x))
    with pytest.raises(NotImplementedError):
        tr.train(None)
