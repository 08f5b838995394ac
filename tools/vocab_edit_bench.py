#!/usr/bin/env python3
"""Vocabulary edits against regenerating the vocabulary ("Editing a generated vocabulary"), one process: a ViT-B/16
model, a 1000 x 16 reference bank, resident synthetic images.  Timed: CustomCLIP.add_classes of 10 classes x 16 images,
remove_classes of those 10, load_bank of the 1000-class bank from a file, and -- the baseline, code this feature does not touch --
forward_prompt on the 1010-class union.  The project's method: HIP events on the launch stream, median of 20 calls after 5 (an edit's
host work lies between the two events, so the figure is the edit's wall time as the stream sees it); no file is written by the timed calls.

    python tools/vocab_edit_bench.py [--classes 1000] [--shots 16] [--add 10] [--model ViT-B/16] [--batch 512]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ovmr_amd import modules, synth
from ovmr_amd.data import ResidentEvalSet

ap = argparse.ArgumentParser()
ap.add_argument("--classes", type=int, default=1000)
ap.add_argument("--shots", type=int, default=16)
ap.add_argument("--add", type=int, default=10)
ap.add_argument("--model", default="ViT-B/16")
ap.add_argument("--batch", type=int, default=512, help="DATALOADER.TEST.BATCH_SIZE: images per loader batch")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--calls", type=int, default=20)
a = ap.parse_args()
spec = synth.SPECS[a.model]
C, S, K, R = a.classes, a.shots, a.add, spec.image_resolution
cpb = max(1, a.batch // S)

clip = modules.CLIPModel({k: torch.from_numpy(v) for k, v in synth.clip_state_dict(spec, 1).items()}, spec)
pl = {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, 2, 1).items()}
tok = torch.zeros(C + K, spec.context_length, dtype=torch.long)          # "a <name>.", names of 1 to 4 tokens, the first one the class's own
a_id, dot_id = (int(t) for t in synth.template_token_ids()[0, 1:3])
for c in range(C + K):
    row = [synth.SOT_ID, a_id, 1000 + c] + [20000 + (7 * c + j) % 9000 for j in range(c % 4)] + [dot_id, synth.EOT_ID]
    tok[c, :len(row)] = torch.tensor(row)
g = torch.Generator(device="cuda").manual_seed(1)
img = torch.randn((C + K) * S, 3, R, R, generator=g, device="cuda", dtype=torch.float16)
old_set = ResidentEvalSet(img[:C * S], torch.arange(C), S, cpb)
new_set = ResidentEvalSet(img[C * S:], torch.arange(K), S, cpb)
union_set = ResidentEvalSet(img, torch.arange(C + K), S, cpb)


def model(rows):
    cfg = modules.make_cfg(n_ctx=2, num_shots=S, output_dir="", backbone=a.model, test_batch_size=a.batch, size=R)
    return modules.CustomCLIP(cfg, rows, clip, prompt_learner_state=pl, reserve=(a.batch, 256, max(1024, C + K)), stream_text=True)


def timed(fn, undo=None):
    ms = []
    for i in range(a.warmup + a.calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        if i >= a.warmup:
            ms.append(t0.elapsed_time(t1))
        if undo is not None:
            undo()
    return round(statistics.median(ms), 3)


out = {"model": a.model, "classes": C, "shots": S, "added": K, "loader_batch": a.batch}
m = model(tok[:C])
m.forward_prompt(old_set)
with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, "reference_bank.pt")
    m.save_bank(path)
    out["bank_mb"] = round(os.path.getsize(path) / 2 ** 20, 1)
    out["load_bank_ms"] = timed(lambda: m.load_bank(path))
new_labels = list(range(C, C + K))
out["add_classes_ms"] = timed(lambda: m.add_classes(tok[C:], new_set), undo=lambda: m.remove_classes(new_labels))
m.add_classes(tok[C:], new_set)
out["remove_classes_ms"] = timed(lambda: m.remove_classes(new_labels), undo=lambda: m.add_classes(tok[C:], new_set))
edited = m.bank_state()
u = model(tok)
out["forward_prompt_union_ms"] = timed(lambda: u.forward_prompt(union_set))
scratch = u.bank_state()
out["edited_equals_from_scratch"] = all(torch.equal(edited[k], scratch[k]) for k in ("features", "visual_tokens", "xval_counts", "fusion_weight"))
out["union_images_per_s"] = round((C + K) * S / out["forward_prompt_union_ms"] * 1e3)
out["add_speedup"] = round(out["forward_prompt_union_ms"] / out["add_classes_ms"], 1)
print(json.dumps(out))
