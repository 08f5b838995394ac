#!/usr/bin/env python3
"""EVAL_MODE all end to end on resident data: the test pass of bench.py's `--preset c3` shape (ViT-B/16, batch 256, 1000 classes,
16 384 query images) -- CustomCLIP.forward_batches + one Classification per mode, as trainer._EvalTrainer.test() runs it -- with
EVAL_MODE all beside EVAL_MODE fusion and beside the four single-mode passes it replaces.  Prints one JSON line: images/s of each
(an image counts once per pass; `four_passes` is 16 384 images over the sum of the four passes' times).

    python tools/all_modes_bench.py [--queries 16384] [--resident 4096] [--batch 256] [--classes 1000] [--passes 3]
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from ovmr_amd import modules, synth
from ovmr_amd.evaluator import Classification
from ovmr_amd.runtime import ALL_MODES

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="ViT-B/16")
ap.add_argument("--queries", type=int, default=16384)
ap.add_argument("--resident", type=int, default=4096, help="distinct images on the device; a pass walks them queries / resident times")
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--classes", type=int, default=1000)
ap.add_argument("--passes", type=int, default=3, help="timed passes per mode after one warm-up pass; the median is reported")
args = ap.parse_args()

spec = synth.SPECS[args.model]
C, D, R = args.classes, spec.embed_dim, spec.image_resolution
cm = modules.CLIPModel({k: torch.from_numpy(v) for k, v in synth.clip_state_dict(spec, 11, jitter=True).items()}, spec)
cfg = modules.make_cfg(n_ctx=2, num_shots=16, output_dir="", test_batch_size=args.batch)
pl = {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, 2, 11, True).items()}
model = modules.CustomCLIP(cfg, torch.from_numpy(synth.class_token_ids(C, seed=9)), cm, prompt_learner_state=pl, reserve=(args.batch, 64, C),
                           stream_text=True)
g = torch.Generator(device="cuda").manual_seed(8)
# the head's cost does not depend on what the classifiers hold: unit rows stand in for generated ones (generation is set-up in c3)
unit = lambda: torch.nn.functional.normalize(torch.randn((C, D), generator=g, device="cuda"), dim=-1).half()
model.mm_classifier, model.visual_classifer, model.zero_shot_classifier = unit(), unit(), unit()
model.fusion_weight = torch.softmax(torch.randn((C, 3), generator=g, device="cuda"), -1)
q = torch.randn((args.resident, 3, R, R), generator=g, device="cuda").half()
labels = torch.randint(0, C, (args.resident,), generator=g, device="cuda")
rounds = max(1, args.queries // args.resident)


def batches():
    for _ in range(rounds):
        for s in range(0, args.resident, args.batch):
            yield s


def one_pass(mode):
    model.cfg.EVAL_MODE = mode
    evs = [Classification(C, device="cuda") for _ in (ALL_MODES if mode == "all" else (mode,))]
    starts = list(batches())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = model.forward_batches((q[s:s + args.batch] for s in starts), stable_inputs=True)
    for s, out in zip(starts, outs):
        for ev, plane in zip(evs, out if out.dim() == 3 else (out,)):
            ev.process(plane, labels[s:s + args.batch])
    counts = [ev.counts() for ev in evs]                 # the host reads the histograms once per evaluator (evaluate())
    dt = time.perf_counter() - t0
    assert all(int(c[2].sum()) == rounds * args.resident for c in counts)
    return dt


def median_pass(mode):
    one_pass(mode)
    return sorted(one_pass(mode) for _ in range(args.passes))[args.passes // 2]


n = rounds * args.resident
t = {mode: median_pass(mode) for mode in ("all",) + ALL_MODES}
four = sum(t[m] for m in ALL_MODES)
print(json.dumps({"model": args.model, "batch": args.batch, "classes": C, "images_per_pass": n, "passes": args.passes,
                  "all_images_per_s": round(n / t["all"], 1), "fusion_images_per_s": round(n / t["fusion"], 1),
                  "four_passes_images_per_s": round(n / four, 1),
                  "ms": {k: round(1000 * v, 2) for k, v in {**t, "four_passes": four}.items()},
                  "speedup_over_four_passes": round(four / t["all"], 3)}), flush=True)
