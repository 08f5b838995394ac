"""BASELINE.json configurations on the HIP path (`pytest -m gpu`), each against the CPU oracle:

  headline  ViT-B/16, 1000 classes x 16 shots + queries: the exact job bench.py times (device-generated weights),
            sampled classes / queries against the oracle, ALL argmax counters against a CPU restatement;
  c4        a vocabulary of >= 5000 classes in ONE process (the reference leaves zero_shot_classifier = None at
            trainers/mm_classifier_one_prompt.py:118 and then fails at :265), cross-validation logits streamed in
            several workspace chunks;
  c5        the classifier-generation head at embed_dim = transformer_width = 768 (ViT-L/14 text side: 12 heads,
            fp32 aggregator 768 wide) through generation and the four EVAL_MODEs.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import usable_threads, COS_TOL, assert_cosine, near_tie_classes
from ovmr_amd import synth

pytestmark = pytest.mark.gpu
SEED = 11
PINNED_MIN = 0.9          # share of the headline job's classes whose six argmax counters the CPU restatement fixes to one value


@pytest.fixture(scope="module")
def O():
    from oracle import ovmr_oracle
    return ovmr_oracle


def _ulp_margin(logits, ulps=3):
    """Per-row margin of `ulps` fp16 steps AT the row maximum: two correct implementations of h(h(f . c) * scale) differ by the
    accumulation order of the dot product, i.e. by one step of h(acc), carried through the second rounding -- at most 2 steps of the
    result; 3 leaves slack.  (0.13 = 2 steps at |logit| in [64, 128): the fixed margin the larger jobs use.)"""
    top = np.abs(logits.max(1, keepdims=True)).astype(np.float16)
    return ulps * np.spacing(np.maximum(top, np.float16(2.0 ** -10))).astype(np.float32)


def _count_bounds(logits, row_labels, C, margin):
    """[lo, hi] for tp and n_pred of every class when an argmax may land on any class within `margin` (a scalar, or one value per
    row as [R, 1]) of the row maximum."""
    top = logits.max(1, keepdims=True)
    cand = logits >= top - margin
    sure = cand.sum(1) == 1
    pred = logits.argmax(1)
    n_lo = np.bincount(pred[sure], minlength=C)
    n_hi = n_lo + cand[~sure].sum(0)
    own = cand[np.arange(len(row_labels)), row_labels]
    tp_lo = np.bincount(row_labels[sure & own], minlength=C)
    tp_hi = tp_lo + np.bincount(row_labels[~sure & own], minlength=C)
    return tp_lo, tp_hi, n_lo, n_hi


def _fp16_logits(feats, clf, scale):
    """h(h(f . c) * scale): the reference's fp16 einsum followed by the 0-dim fp32 scale (:263-265), from fp32 sums."""
    return ((feats.float() @ clf.float().t()).half().float() * scale).half().float().numpy()


@pytest.mark.timeout(1800)
def test_headline_config_bench_job_vs_oracle(O):
    """The job bench.py times -- ViT-B/16, 1000 classes x 16 shots, weights drawn on the device exactly as bench.py
    draws them -- through CustomCLIP.forward_prompt on the HIP path, then
      * 4 sampled classes: image features, multimodal / vision / text classifier rows and visual tokens against the oracle
        (64 images + 12 prompts of CPU work),
      * ALL 3 x 2 x 1000 argmax counters against a CPU restatement on the same fp16 features / classifier rows
        (an argmax may land on any class within 3 fp16 steps of the row maximum: bounds per counter); the number of classes whose
        counters the bounds pin to a single value is printed and must be at least 90 %,
      * fusion weights = softmax(tau * F1(counters)) exactly,
      * 8 query rows of the fused output against the oracle."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from ovmr_amd import modules
    from ovmr_amd.data import ResidentEvalSet
    dev = torch.device("cuda:0")
    spec, C, S, n_ctx, batch = synth.SPECS["ViT-B/16"], 1000, 16, 2, bench.DEFAULT_BATCH   # bench.py defaults: --batch 775, --classes-per-batch 1000
    gen = torch.Generator(device=dev).manual_seed(1234)
    sd = bench.device_clip_state(spec, gen, dev)
    pl = bench.device_pl_state(spec, n_ctx, gen, dev)
    cm = modules.CLIPModel(sd, spec, str(dev))
    cfg = modules.make_cfg(n_ctx=n_ctx, num_shots=S, eval_mode="fusion", eval_tau=10.0, output_dir="", test_batch_size=batch)
    tok = torch.from_numpy(synth.class_token_ids(C, seed=4321))
    model = modules.CustomCLIP(cfg, tok, cm, prompt_learner_state=pl, reserve=(batch, 1024, 1024))
    ig = torch.Generator(device=dev).manual_seed(1234)
    R = spec.image_resolution
    ex = torch.empty((C * S, 3, R, R), dtype=torch.float16, device=dev)
    for s in range(0, C * S, 1024):
        ex[s:s + 1024] = torch.randn((min(1024, C * S - s), 3, R, R), generator=ig, device=dev).half()
    q = torch.randn((8, 3, R, R), generator=ig, device=dev).half()
    loader = ResidentEvalSet(ex, torch.arange(C, device=dev), S, bench.DEFAULT_CLASSES_PER_BATCH, presharded=True)
    mm, v, fw = model.forward_prompt(loader)
    out = model(q).cpu()
    t = model.zero_shot_classifier
    feats = model.eval_feat4cls
    assert bool(torch.isfinite(mm.float()).all() and torch.isfinite(v.float()).all() and torch.isfinite(fw).all())

    # ---- sampled classes against the oracle (CPU, fp16 like the reference)
    cpu_sd = O.convert_weights({k: x.detach().float().cpu() for k, x in sd.items()}, "fp16")
    cpu_pl = {k: x.detach().float().cpu() for k, x in pl.items()}
    sample = [0, 333, 642, 999]
    torch.set_num_threads(usable_threads())
    rows = torch.cat([ex[c * S:(c + 1) * S] for c in sample]).cpu()
    with torch.no_grad():
        r = O.forward_prompt(rows, torch.arange(len(sample)).repeat_interleave(S), tok[sample], cpu_sd, cpu_pl, n_ctx, 10.0,
                             len(sample), "fp16")
        qf = O.l2_normalize(O.encode_image(q.cpu(), cpu_sd))
    assert_cosine(feats[sample].flatten(0, 1).float().cpu().numpy(), r["eval_feat4cls"].flatten(0, 1).float().numpy(), COS_TOL, "eval_feat4cls")
    assert_cosine(mm[sample].float().cpu().numpy(), r["mm_classifier"].numpy(), COS_TOL, "mm rows")
    assert_cosine(v[sample].float().cpu().numpy(), r["vision_classifier"].numpy(), COS_TOL, "vision rows")
    assert_cosine(t[sample].float().cpu().numpy(), r["text_classifier"].numpy(), COS_TOL, "text rows")
    assert_cosine(model.visual_tokens[sample].float().cpu().numpy(), r["visual_tokens"].float().numpy(), COS_TOL, "visual tokens")

    # ---- every counter of the cross-validation step, on the job's own fp16 features and classifier rows
    counts = model.xval_counts.cpu().numpy()
    f_cpu = feats.flatten(0, 1).cpu()
    row_lab = np.repeat(np.arange(C), S)
    ls = float(model.engine.logit_scale)
    pinned = np.ones(C, dtype=bool)                  # classes whose six counters the restatement fixes to ONE value (no near-tie can reach them)
    for m, clf in enumerate((mm, v, t)):
        lg = _fp16_logits(f_cpu, clf.cpu(), ls)
        tp_lo, tp_hi, n_lo, n_hi = _count_bounds(lg, row_lab, C, _ulp_margin(lg))      # 3 fp16 steps at each row's own maximum
        assert counts[m, 1].sum() == C * S
        assert ((counts[m, 0] >= tp_lo) & (counts[m, 0] <= tp_hi)).all(), f"tp of classifier {m}"
        assert ((counts[m, 1] >= n_lo) & (counts[m, 1] <= n_hi)).all(), f"n_pred of classifier {m}"
        pinned &= (tp_lo == tp_hi) & (n_lo == n_hi)
        print(f"  classifier {m}: row maxima {float(lg.max(1).min()):.2f} .. {float(lg.max(1).max()):.2f}, "
              f"{int((tp_lo == tp_hi).sum())} tp / {int((n_lo == n_hi).sum())} n_pred counters pinned")
    # how much of the job the bounds pin EXACTLY: for these classes lo == hi, i.e. the HIP counters equal the CPU restatement's
    print(f"headline job: {int(pinned.sum())} of {C} classes have all six counters pinned exactly (no argmax within 3 fp16 steps of a row maximum touches them)")
    assert pinned.sum() >= PINNED_MIN * C, f"only {int(pinned.sum())} of {C} classes are pinned exactly"
    f1 = torch.stack([O.f1_from_counts(torch.from_numpy(counts[m, 0]), torch.from_numpy(counts[m, 1]), torch.full((C,), S))
                      for m in range(3)], -1)
    np.testing.assert_allclose(fw.cpu().numpy(), (10.0 * f1).softmax(-1).numpy(), atol=1e-6)

    # ---- fused query rows: oracle features, the job's classifiers and weights
    ref = O.inference_logits(qf, mm.cpu(), v.cpu(), t.cpu(), fw.cpu(), torch.tensor(ls), "fusion")
    assert out.shape == (8, C)
    assert_cosine(out.numpy(), ref.numpy(), COS_TOL, "fused query rows")
    del model, cm, ex
    torch.cuda.empty_cache()


def _small_clip(name, gain=0.0):
    from ovmr_amd import modules
    spec = synth.SPECS[name]
    sd = synth.clip_state_dict(spec, SEED, jitter=True)
    pl = synth.prompt_learner_state_dict(spec, 2, SEED, True)
    if gain:
        synth.align_state_dicts(sd, pl, spec, gain)
    cm = modules.CLIPModel({k: torch.from_numpy(x) for k, x in sd.items()}, spec)
    return spec, sd, pl, cm


@pytest.mark.timeout(1800)
def test_config_c4_six_thousand_classes_single_process(O, tmp_path):
    """C = 6000 >= 5000 in one process on the tiny model, 2 shots: the text rows are encoded batch by batch (the reference
    cannot run this at all), the cross-validation logits [12000, 6000] = 72 M elements stream through the 32 M-element
    workspace in three chunks.  Classifier rows against the oracle on sampled classes; all counters against the CPU
    restatement and against the same kernel fed 1000 rows at a time (chunk-boundary independence)."""
    from ovmr_amd import modules
    spec, sd, pl, cm = _small_clip("tiny")
    C, S, cpb = 6000, 2, 500
    tok = torch.from_numpy(synth.class_token_ids(C, seed=77))
    cfg = modules.make_cfg(n_ctx=2, num_shots=S, output_dir=str(tmp_path))
    model = modules.CustomCLIP(cfg, tok, cm, prompt_learner_state={k: torch.from_numpy(x) for k, x in pl.items()},
                               reserve=(1024, 1024, 1024))
    assert model.zero_shot_classifier is None                       # :118 -- lifted inside forward_prompt
    g = torch.Generator().manual_seed(9)
    order = torch.randperm(C, generator=g)
    labels = order.repeat_interleave(S)
    pat = torch.randn((C, 3, 32, 32), generator=g)
    img = 0.6 * torch.randn((C * S, 3, 32, 32), generator=g) + 0.8 * pat[labels]
    loader = [{"img": img[s:s + cpb * S], "label": labels[s:s + cpb * S]} for s in range(0, C * S, cpb * S)]
    mm, v, fw = model.forward_prompt(loader)
    t = model.zero_shot_classifier
    assert t is not None and t.shape == (C, spec.embed_dim) and fw.shape == (C, 3)
    saved = torch.load(os.path.join(str(tmp_path), "mm_classifiers.pt"), map_location="cpu")
    assert saved["text_classifier"].shape == (C, spec.embed_dim) and saved["text_classifier"].dtype == torch.float32

    sample = torch.tensor([0, 17, 2999, 4999, 5000, 5999])
    cpu_sd = O.convert_weights(O.to_torch(sd), "fp16")
    rows = torch.cat([img[(labels == c)] for c in sample.tolist()])
    with torch.no_grad():
        r = O.forward_prompt(rows, torch.arange(len(sample)).repeat_interleave(S), tok[sample], cpu_sd, O.to_torch(pl), 2, 10.0,
                             len(sample), "fp16")
    assert_cosine(mm[sample].float().cpu().numpy(), r["mm_classifier"].numpy(), COS_TOL, "mm rows")
    assert_cosine(v[sample].float().cpu().numpy(), r["vision_classifier"].numpy(), COS_TOL, "vision rows")
    assert_cosine(t[sample].float().cpu().numpy(), r["text_classifier"].numpy(), COS_TOL, "text rows")

    counts = model.xval_counts.cpu().numpy()
    feats = model.eval_feat4cls.flatten(0, 1)
    row_lab_t = torch.arange(C, dtype=torch.int32).repeat_interleave(S)
    row_lab = row_lab_t.numpy()
    ls = float(model.engine.logit_scale)
    for m, clf in enumerate((mm, v, t)):
        lg = _fp16_logits(feats.cpu(), clf.cpu(), ls)
        tp_lo, tp_hi, n_lo, n_hi = _count_bounds(lg, row_lab, C, 0.13)
        assert counts[m, 1].sum() == C * S
        assert ((counts[m, 0] >= tp_lo) & (counts[m, 0] <= tp_hi)).all(), f"tp of classifier {m}"
        assert ((counts[m, 1] >= n_lo) & (counts[m, 1] <= n_hi)).all(), f"n_pred of classifier {m}"
        # the same rows 1000 at a time: identical counters
        again = torch.zeros((2, C), dtype=torch.int32, device="cuda")
        for r0 in range(0, C * S, 1000):
            model.engine.xval_counts(feats[r0:r0 + 1000], row_lab_t[r0:r0 + 1000], clf, again[0], again[1])
        np.testing.assert_array_equal(again.cpu().numpy(), counts[m])
    f1 = torch.stack([O.f1_from_counts(torch.from_numpy(counts[m, 0]), torch.from_numpy(counts[m, 1]), torch.full((C,), S))
                      for m in range(3)], -1)
    np.testing.assert_allclose(fw.cpu().numpy(), (10.0 * f1).softmax(-1).numpy(), atol=1e-6)
    # fused inference at C = 6000 against the oracle on the job's own classifiers
    q = img[:5]
    out = model(q).cpu()
    with torch.no_grad():
        qf = O.l2_normalize(O.encode_image(q.half(), cpu_sd))
    ref = O.inference_logits(qf, mm.cpu(), v.cpu(), t.cpu(), fw.cpu(), torch.tensor(ls), "fusion")
    assert_cosine(out.numpy(), ref.numpy(), COS_TOL, "fused rows at C = 6000")


@pytest.mark.timeout(3000)
def test_config_c4_vitb16_sixty_four_shots_one_rank_of_eight(O):
    """BASELINE.json configuration 4 on its own architecture: ViT-B/16, 64 shots (aggregator sequence 66 behind the real image
    tower), a 5040-class vocabulary (>= 5000: the reference leaves zero_shot_classifier = None at
    trainers/mm_classifier_one_prompt.py:118 and fails at :263-265), class-sharded over 8 ranks -- the job `bench.py --preset c4`
    runs (bench.shard_of_world), at 5040 instead of 10 000 classes: the exemplars of rank 0 and of two sampled peers (ranks 5 and 7: 120 960
    images, 630 classes each; the bench preset and --emulate-world run all eight ranks' through the encoder) go through hot loop A, the
    other five ranks contribute random unit rows and features under their own labels; rank 0 then runs the SHARDED path with the peers'
    recorded rows and votes.  Checked:
      * rank 0 ends with the whole job's bits (rows, tokens, counters, fusion weights) -- asserted inside shard_of_world;
      * 3 sampled classes (2 of rank 0, 1 of rank 5): features, mm / vision / text rows, visual tokens against the oracle;
      * ALL 3 x 2 x 5040 counters of the whole job AND rank 0's own votes against the CPU restatement's bounds, 8 064 rows at a time
        (an argmax may land on any class within 3 fp16 steps of the row maximum; the share of classes pinned to one value is printed, >= 90 %);
      * fusion weights = softmax(tau * F1(counters)) exactly;
      * the four EVAL_MODEs on 8 queries against the oracle (oracle features, the job's classifiers and weights)."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from ovmr_amd.shard import shard_range
    dev = torch.device("cuda:0")
    C, S, N = 5040, 64, 8
    args = bench.parse(["--preset", "c4", "--classes", str(C), "--classes-per-batch", str(C // N), "--queries", "2048",
                        "--steps", "1", "--warmup", "0", "--full", "--no-cpu-baseline"])
    assert args.shots == S and args.emulate_world == N and args.model == "ViT-B/16"
    spec, sd, pl, tok, model = bench.make_model(args, dev)
    assert model.zero_shot_classifier is None or model._text_streamed
    keep = {}
    # rank 0 (timed, through the sharded path) and two sampled peers (5: checked against the oracle below; 7: the last, ragged-free shard)
    # run their exemplars through the encoder; the other five ranks contribute random unit rows / features under their own labels.  All
    # eight ranks through the encoder, every one bit-equal to the whole job: bench.py --preset c4 and --emulate-world 8 (profiles/).
    line = bench.shard_of_world(args, model, spec, dev, keep, peers=[5, 7])
    assert line["projection"]["projected"] and all(line["projection"]["rank_reproduces_whole_job_bits"].values())
    assert line["config"]["images_per_step"] == (C // N) * S + 2048 // N and line["value"] > 0
    ref, counts_full, feats = keep["ref"], keep["counts_full"].cpu().numpy(), keep["eval_feat4cls"]
    mm, v, t, fw = ref["mm_classifier"], ref["visual_classifer"], ref["zero_shot_classifier"], ref["fusion_weight"]
    assert mm.shape == (C, 512) and fw.shape == (C, 3)
    assert bool(torch.isfinite(mm.float()).all() and torch.isfinite(v.float()).all() and torch.isfinite(t.float()).all() and torch.isfinite(fw).all())

    # ---- sampled classes against the oracle: two of rank 0 (its exemplars are still resident), the first class of rank 5 (redrawn)
    cpu_sd = O.convert_weights({k: x.detach().float().cpu() for k, x in sd.items()}, "fp16")
    cpu_pl = {k: x.detach().float().cpu() for k, x in pl.items()}
    R = spec.image_resolution
    ex0 = keep["exemplars"]
    c5 = shard_range(C, 5, N)[0]
    ig = torch.Generator(device=dev).manual_seed(1234 + 5)
    first = torch.randn((1024, 3, R, R), generator=ig, device=dev).half()
    sample = [0, 629, c5]
    rows = torch.cat([ex0[0:S], ex0[629 * S:630 * S], first[:S]]).cpu()
    torch.set_num_threads(usable_threads())
    with torch.no_grad():
        r = O.forward_prompt(rows, torch.arange(3).repeat_interleave(S), tok[sample], cpu_sd, cpu_pl, 2, 10.0, 3, "fp16")
        qf = O.l2_normalize(O.encode_image(keep["queries"][:8].cpu(), cpu_sd))
    assert_cosine(feats[sample].flatten(0, 1).float().cpu().numpy(), r["eval_feat4cls"].flatten(0, 1).float().numpy(), COS_TOL, "eval_feat4cls")
    assert_cosine(mm[sample].float().cpu().numpy(), r["mm_classifier"].numpy(), COS_TOL, "mm rows")
    assert_cosine(v[sample].float().cpu().numpy(), r["vision_classifier"].numpy(), COS_TOL, "vision rows")
    assert_cosine(t[sample].float().cpu().numpy(), r["text_classifier"].numpy(), COS_TOL, "text rows")
    assert_cosine(ref["visual_tokens"][sample].float().cpu().numpy(), r["visual_tokens"].float().numpy(), COS_TOL, "visual tokens")

    # ---- every counter, whole job and rank 0's own votes, in row chunks (the bounds add up over rows)
    f_cpu = feats.flatten(0, 1).cpu()
    ls = float(model.engine.logit_scale)
    local_counts = keep["local_counts"].cpu().numpy()
    n_local = (C // N) * S
    chunk = 8064                                                                  # 126 classes: rank boundaries fall on chunk boundaries
    assert n_local % chunk == 0
    pinned = np.ones(C, dtype=bool)
    for m, clf in enumerate((mm, v, t)):
        clf_cpu = clf.cpu()
        acc = np.zeros((4, C), dtype=np.int64)
        for r0 in range(0, C * S, chunk):
            row_lab = np.repeat(np.arange(r0 // S, (r0 + chunk) // S), S)
            if r0 // n_local not in (0, 5, 7):
                # a stand-in rank (shard_of_world peers=): its rows vote for their own class by construction -- established here on the
                # device (top-2 margin > 1 where 3 fp16 steps are < 0.2), so the CPU restatement of 40 320 x 5 040 logits is spared
                lgd = (feats.flatten(0, 1)[r0:r0 + chunk].float() @ clf.float().t()) * ls
                top2 = lgd.topk(2, dim=1)
                assert float((top2.values[:, 0] - top2.values[:, 1]).min()) > 1.0
                assert bool((top2.indices[:, 0].cpu() == torch.from_numpy(row_lab)).all())
                acc += np.bincount(row_lab, minlength=C)[None, :]
                continue
            lg = _fp16_logits(f_cpu[r0:r0 + chunk], clf_cpu, ls)
            acc += np.stack(_count_bounds(lg, row_lab, C, _ulp_margin(lg)))
            if r0 + chunk == n_local:
                tp_lo, tp_hi, n_lo, n_hi = acc
                assert local_counts[m, 1].sum() == n_local
                assert ((local_counts[m, 0] >= tp_lo) & (local_counts[m, 0] <= tp_hi)).all(), f"rank 0 tp of classifier {m}"
                assert ((local_counts[m, 1] >= n_lo) & (local_counts[m, 1] <= n_hi)).all(), f"rank 0 n_pred of classifier {m}"
        tp_lo, tp_hi, n_lo, n_hi = acc
        assert counts_full[m, 1].sum() == C * S
        assert ((counts_full[m, 0] >= tp_lo) & (counts_full[m, 0] <= tp_hi)).all(), f"tp of classifier {m}"
        assert ((counts_full[m, 1] >= n_lo) & (counts_full[m, 1] <= n_hi)).all(), f"n_pred of classifier {m}"
        pinned &= (tp_lo == tp_hi) & (n_lo == n_hi)
    f1 = torch.stack([O.f1_from_counts(torch.from_numpy(counts_full[m, 0]), torch.from_numpy(counts_full[m, 1]), torch.full((C,), S))
                      for m in range(3)], -1)
    np.testing.assert_allclose(fw.cpu().numpy(), (10.0 * f1).softmax(-1).numpy(), atol=1e-6)

    # ---- the four EVAL_MODEs on 8 queries
    q8 = keep["queries"][:8]
    m = keep["model"]
    want = O.inference_logits(qf, mm.cpu(), v.cpu(), t.cpu(), fw.cpu(), torch.tensor(ls), "fusion")
    assert_cosine(keep["out"][:8].cpu().numpy(), want.numpy(), COS_TOL, "fusion rows of the timed query loop (batch 256, two in flight)")
    for mode in ("fusion", "text", "vision", "multimodal"):
        m.cfg.EVAL_MODE = mode
        out = m(q8).cpu()
        want = O.inference_logits(qf, mm.cpu(), v.cpu(), t.cpu(), fw.cpu(), torch.tensor(ls), mode)
        assert out.shape == (8, C)
        assert_cosine(out.numpy(), want.numpy(), COS_TOL, f"{mode} rows at C = {C}")
    m.cfg.EVAL_MODE = "fusion"
    print(f"c4 job: {int(pinned.sum())} of {C} classes have all six counters pinned exactly")
    assert pinned.sum() >= PINNED_MIN * C
    print(f"c4 at ViT-B/16: rank 0 of {N}: {line['value']:.0f} img/s, generation {line['phases']['generation_images_per_s']:.0f} img/s, "
          f"xval {line['phases']['xval_counts_fusion_weights_ms']:.2f} ms")
    del keep, model, m
    torch.cuda.empty_cache()


def test_config_c5_head_at_width_768(O, tmp_path):
    """embed_dim = transformer_width = 768 (the ViT-L/14 head: 12 text heads, fp32 aggregator 768 wide with 12 heads,
    prompts assembled at width 768, cross-validation / fused logits at K = 768) on a 2-layer model: generation and the
    four EVAL_MODEs against the oracle, 12 classes x 32 shots (config 5's shot count: aggregator sequence 34)."""
    from ovmr_amd import modules
    spec, sd, pl, cm = _small_clip("head768", gain=3.0)
    C, S, cpb, tau = 12, 32, 5, 3.0
    tok = torch.from_numpy(synth.class_token_ids(C, seed=5))      # seed picked (offline, with the oracle) for clear text argmaxes
    cfg = modules.make_cfg(n_ctx=2, num_shots=S, eval_tau=tau, output_dir=str(tmp_path))
    model = modules.CustomCLIP(cfg, tok, cm, prompt_learner_state={k: torch.from_numpy(x) for k, x in pl.items()},
                               reserve=(256, 64, 64))
    labels = np.repeat(np.random.default_rng(5).permutation(C), S)
    img = torch.from_numpy(synth.images(C * S, spec.image_resolution, 1234, labels, 0.9, tile=16))
    qlab = np.arange(8) % C
    q = torch.from_numpy(synth.images(8, spec.image_resolution, 777, qlab, 0.9, tile=16))
    loader = [{"img": img[s:s + cpb * S], "label": torch.from_numpy(labels[s:s + cpb * S])} for s in range(0, C * S, cpb * S)]
    outs = {}
    for mode in ("fusion", "text", "vision", "multimodal"):
        cfg.EVAL_MODE = mode
        outs[mode] = model(q, eval_set_loader=loader).cpu()
    cpu_sd = O.convert_weights(O.to_torch(sd), "fp16")
    with torch.no_grad():
        r = O.forward_prompt(img, torch.from_numpy(labels), tok, cpu_sd, O.to_torch(pl), 2, tau, cpb, "fp16")
        qf = O.l2_normalize(O.encode_image(q.half(), cpu_sd))
    assert_cosine(model.eval_feat4cls.float().cpu().numpy(), r["eval_feat4cls"].float().numpy(), COS_TOL, "eval_feat4cls")
    np.testing.assert_allclose(model.visual_tokens.float().cpu().numpy(), r["visual_tokens"].float().numpy(), atol=2e-2, rtol=2e-2)
    assert_cosine(model.visual_tokens.float().cpu().numpy(), r["visual_tokens"].float().numpy(), COS_TOL, "visual tokens")
    assert_cosine(model.mm_classifier.float().cpu().numpy(), r["mm_classifier"].numpy(), COS_TOL, "mm")
    assert_cosine(model.visual_classifer.float().cpu().numpy(), r["vision_classifier"].numpy(), COS_TOL, "vision")
    assert_cosine(model.zero_shot_classifier.float().cpu().numpy(), r["text_classifier"].numpy(), COS_TOL, "text")
    ls = cpu_sd["logit_scale"].float().exp()
    affected = set()
    for k in ("mm_classifier", "vision_classifier", "text_classifier"):
        affected |= near_tie_classes(O.cross_validation_logits(r["eval_feat4cls"], r[k].half(), ls).float().numpy(), 0.26)
    ok = np.array([c not in affected for c in range(C)])
    assert ok.sum() >= C - 3, f"only {int(ok.sum())} classes free of near-ties"
    np.testing.assert_allclose(model.fusion_weight.cpu().numpy()[ok], r["fusion_weight"].numpy()[ok], atol=1e-5)
    for mode in ("text", "vision", "multimodal"):
        ref = O.inference_logits(qf, r["mm_classifier"].half(), r["vision_classifier"].half(), r["text_classifier"].half(),
                                 r["fusion_weight"], ls, mode)
        assert_cosine(outs[mode].numpy(), ref.numpy(), COS_TOL, mode)
    ref = O.inference_logits(qf, r["mm_classifier"].half(), r["vision_classifier"].half(), r["text_classifier"].half(),
                             r["fusion_weight"], ls, "fusion")
    assert_cosine(outs["fusion"].numpy()[:, ok], ref.numpy()[:, ok], COS_TOL, "fusion (classes free of near-ties)")


def test_forward_batches_equals_forward_with_two_batches_in_flight(tmp_path):
    """CustomCLIP.forward_batches (the test loop's forwards on two handles / two streams): every batch's logits bit-equal to
    forward() on that batch, in order -- with resident inputs, with a loader that RECYCLES two device buffers (the pipelined
    folder loader's behaviour: the buffer of batch i is overwritten as soon as batch i + 1 has been asked for), with a ragged
    last batch, with a batch above the overlap limit (falls back to the single handle), and after an option change and a
    prompt-learner reload on the first handle (the twin follows)."""
    from ovmr_amd import modules
    spec, sd, pl, cm = _small_clip("tiny", gain=2.0)
    C, S, B = 12, 4, 24
    tok = torch.from_numpy(synth.class_token_ids(C, seed=5))
    cfg = modules.make_cfg(n_ctx=2, num_shots=S, output_dir=str(tmp_path))
    model = modules.CustomCLIP(cfg, tok, cm, prompt_learner_state={k: torch.from_numpy(x) for k, x in pl.items()}, reserve=(64, 64, 64))
    model.OVERLAP_MAX_BATCH = 32
    g = torch.Generator().manual_seed(3)
    R = spec.image_resolution
    labels = torch.arange(C).repeat_interleave(S)
    ex = torch.randn((C * S, 3, R, R), generator=g)
    model.forward_prompt([{"img": ex, "label": labels}])
    q = torch.randn((5 * B + 7, 3, R, R), generator=g).half().cuda()
    chunks = [q[s:s + B] for s in range(0, q.shape[0], B)]
    want = [model(c).clone() for c in chunks]
    torch.cuda.synchronize()

    got = [o.clone() for o in model.forward_batches(iter(chunks), stable_inputs=True)]
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    assert getattr(model, "_twin_engine", None) is not None                    # the second handle was used

    def recycling_loader():
        bufs = [torch.empty((B, 3, R, R), dtype=torch.float16, device="cuda") for _ in range(2)]
        for i, c in enumerate(chunks):
            bufs[i & 1][:c.shape[0]].copy_(c)
            yield bufs[i & 1][:c.shape[0]]
            bufs[i & 1].fill_(float("nan"))                                    # the caller came back: the buffer is fair game

    got = [o.clone() for o in model.forward_batches(recycling_loader())]
    assert all(torch.equal(a, b) for a, b in zip(got, want))

    big = q[:40]                                                               # above the limit: single handle, in order with the rest
    seq = [chunks[0], big, chunks[1]]
    got = [o.clone() for o in model.forward_batches(iter(seq))]
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], model(big)) and torch.equal(got[2], want[1])

    it = model.forward_batches(iter(chunks), stable_inputs=True)               # an abandoned loop: what is in flight is ordered in front of
    first = next(it).clone()                                                   # the next use of the handles on the caller's stream
    next(it)
    it.close()
    assert torch.equal(first, want[0]) and torch.equal(model(chunks[3]), want[3]) and torch.equal(model(chunks[0]), want[0])

    # forward() itself splits a batch of at least 2 x SPLIT_MIN_HALF images over the two handles: the same rows, bit for bit, as one handle
    model.SPLIT_MIN_HALF = 6                                                   # 2 x 6 <= 24 <= 32 (the twin's capacity): split
    split = model(q[:24])
    assert hasattr(model, "_split_stream") and split.shape == (24, C)
    assert torch.equal(split, want[0])                                         # (want[0] was one handle: 24 < 2 x 64)
    assert torch.equal(split, torch.cat([model._forward_on(model.engine, q[:12]), model._forward_on(model.engine, q[12:24])]))
    odd = model(q[:23])                                                        # halves of 12 and 11 rows
    assert torch.equal(odd, want[0][:23])
    model.SPLIT_FORWARD = False
    assert torch.equal(model(q[:24]), want[0])
    model.SPLIT_FORWARD = True
    model.SPLIT_MIN_HALF = 64
    model.engine.set_option("gelu_exact", 1)                                   # the twin mirrors the options of the first handle ...
    want_exact = [model(c).clone() for c in chunks[:3]]
    got = [o.clone() for o in model.forward_batches(iter(chunks[:3]))]
    assert all(torch.equal(a, b) for a, b in zip(got, want_exact))
    model.engine.set_option("gelu_exact", 0)
    twin_before = model._twin_engine
    model.prompt_learner.load_state_dict({k: torch.from_numpy(x) for k, x in pl.items()})   # ... and is rebuilt after a weight reload
    got = [o.clone() for o in model.forward_batches(iter(chunks[:3]))]
    assert model._twin_engine is not twin_before
    assert all(torch.equal(a, b) for a, b in zip(got, want[:3]))


def test_forward_split_keeps_the_unsplit_head_implementation():
    """The head runs as ONE launch for up to 256 rows (512 rows up to 2048 classes) and as GEMMs + softmax beyond (ovmr_head_plan), and the
    two may differ by one fp16 step in a logit.  forward() runs a batch's two halves on two handles only where both halves take the
    implementation the whole batch takes: model(b) == forward with SPLIT_FORWARD = False == forward_batches' output, bit for bit, also for
    300 images against 2500 classes (whole batch: GEMM path; its halves alone would take the one-launch kernel) -- and the split still
    happens, with the same bits, where the plan agrees (300 images against 1000 classes)."""
    from ovmr_amd import modules
    spec, sd, pl, cm = _small_clip("tiny")
    B, D = 300, spec.embed_dim
    g = torch.Generator(device="cuda").manual_seed(8)
    q = torch.randn((B, 3, spec.image_resolution, spec.image_resolution), generator=g, device="cuda").half()
    for C, splits in ((2500, False), (1000, True)):
        tok = torch.from_numpy(synth.class_token_ids(C, seed=9))
        cfg = modules.make_cfg(n_ctx=2, num_shots=2, output_dir="")
        model = modules.CustomCLIP(cfg, tok, cm, prompt_learner_state={k: torch.from_numpy(x) for k, x in pl.items()}, reserve=(B, 64, C),
                                   stream_text=True)
        unit = lambda: torch.nn.functional.normalize(torch.randn((C, D), generator=g, device="cuda"), dim=-1).half()
        model.mm_classifier, model.visual_classifer, model.zero_shot_classifier = unit(), unit(), unit()
        model.fusion_weight = torch.softmax(torch.randn((C, 3), generator=g, device="cuda"), -1)
        e = model.engine
        assert (e.head_plan(B, C), e.head_plan(B // 2, C)) == ((0, 1) if C == 2500 else (1, 1))
        assert model._split_keeps_bits(B) == splits and 2 * model.SPLIT_MIN_HALF <= B <= model._split_cap()
        got = model(q).clone()
        assert hasattr(model, "_split_stream") == splits
        model.SPLIT_FORWARD = False
        want = model(q).clone()
        model.SPLIT_FORWARD = True
        assert torch.equal(got, want)
        (fb,) = [o.clone() for o in model.forward_batches(iter([q]), stable_inputs=True)]
        assert torch.equal(fb, want)
        # what the rule protects against: the two implementations are NOT promised to agree bit for bit
        e.set_option("fused_head", 2 if C == 2500 else 0)
        other = model._forward_on(e, q).clone()
        e.set_option("fused_head", 1)
        assert float((other - want).abs().max()) < 2e-3
        del model
    torch.cuda.empty_cache()


def test_config_c1_zeroshot_bench_line():
    """BASELINE.json configuration 1 as `bench.py --preset c1` runs it (trainers/zsclip.py:32-60 on ViT-B/16, ten prompts): the line's
    fields, the evaluator's invariants on the device-counted test pass, and the logits of the timed loop against a plain model_inference."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    args = bench.parse(["--preset", "c1", "--queries", "640", "--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline"])
    assert (args.model, args.classes, args.query_batch) == ("ViT-B/16", 10, 256)
    line = bench.zeroshot_config(args, torch.device("cuda:0"))
    assert line["unit"] == "images/s" and line["value"] > 0 and line["dtype"] == "f16" and line["config"]["preset"] == "c1"
    assert line["config"]["images_per_step"] == 640 and line["config"]["inference_batches_in_flight"] == 2
    r = line["roofline"]
    assert r["bound"] == "mfma" and 0.0 < r["frac"] < 1.0 and abs(r["achieved"] / r["peak"] - r["frac"]) < 1e-3
    assert 0.0 <= line["phases"]["accuracy_of_random_labels"] <= 100.0 and line["cpu_baseline"] is None
    torch.cuda.empty_cache()


def test_generation_synchronises_with_the_host_once(tmp_path):
    """A host synchronisation in the middle of hot loop A is a bubble for everything enqueued behind it (round 6: `buffer[index] = 1` copied its
    scalar from pageable memory in front of ~50 launches of the sharded head -- 0.9 ms of gaps per rank).  With a device-resident exemplar set
    one generation job -- one process, and as rank 1 of 4 through the sharded path with the collectives served from recorded blocks --
    makes the host wait exactly once: the completeness check at its end (trainers/mm_classifier_one_prompt.py:259).  torch's sync debug mode
    reports every call that waits."""
    import warnings
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from ovmr_amd import modules
    from ovmr_amd.data import ResidentEvalSet
    from ovmr_amd.shard import shard_range, local_class_bound
    spec, sd, pl, cm = _small_clip("small")
    C, S, D = 16, 4, spec.embed_dim
    tok = torch.from_numpy(synth.class_token_ids(C, seed=3))
    cfg = modules.make_cfg(n_ctx=2, num_shots=S, output_dir=str(tmp_path))
    model = modules.CustomCLIP(cfg, tok, cm, prompt_learner_state={k: torch.from_numpy(x) for k, x in pl.items()}, reserve=(64, 64, 64), stream_text=True)
    g = torch.Generator(device="cuda").manual_seed(4)
    ex = torch.randn((C * S, 3, spec.image_resolution, spec.image_resolution), generator=g, device="cuda").half()
    q = torch.randn((8, 3, spec.image_resolution, spec.image_resolution), generator=g, device="cuda").half()

    def syncs(fn):
        fn()                                                                   # warm-up: lazy module loads, first-use allocations
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        return [str(x.message) for x in w if "synchroniz" in str(x.message).lower() and "prototype" not in str(x.message).lower()]

    whole = ResidentEvalSet(ex, torch.arange(C, device="cuda"), S, 8, presharded=True)

    def job():
        model.forward_prompt(whole, wait_files=False)
        model(q)
        model.wait_files()

    found = syncs(job)
    assert len(found) == 1, found
    # the test loop itself -- forwards two in flight, every batch counted by the evaluator on the device -- never waits; evaluate() reads once
    from ovmr_amd.evaluator import Classification
    ev = Classification(C, device="cuda")
    labels = torch.randint(0, C, (32,), generator=g, device="cuda")
    batches = [torch.randn((8, 3, spec.image_resolution, spec.image_resolution), generator=g, device="cuda").half() for _ in range(4)]

    def loop():
        for i, out in enumerate(model.forward_batches(iter(batches), stable_inputs=True)):
            ev.process(out, labels[8 * i:8 * i + 8])

    assert syncs(loop) == []
    assert len(syncs(lambda: ev.counts())) == 1
    # rank 1 of 4 through the sharded path (the collectives served on the device: bench.EmulatedPeers)
    c0, c1 = shard_range(C, 1, 4)
    emu = bench.EmulatedPeers(1, 4)
    bound = local_class_bound(C, 4, True, 1)
    emu.peer_blocks = torch.zeros((4 * bound, 5 * D + 2), dtype=torch.float16, device="cuda")
    lab = torch.full((4 * bound,), -1, dtype=torch.int32, device="cuda")
    for r in range(4):
        r0, r1 = shard_range(C, r, 4)
        lab[r * bound:r * bound + (r1 - r0)] = torch.arange(r0, r1, dtype=torch.int32, device="cuda")
    emu.peer_blocks[:, -2:] = lab.view(torch.float16).reshape(-1, 2)
    emu.peer_counts = torch.zeros((3, 2, C), dtype=torch.int32, device="cuda")
    model._dist, model._text_streamed = emu, True
    shard = ResidentEvalSet(ex[c0 * S:c1 * S], torch.arange(c0, c1, device="cuda"), S, 8, presharded=True)
    found = syncs(lambda: (model.forward_prompt(shard, wait_files=False), model(q)))
    model._dist = None
    assert len(found) == 1, found
