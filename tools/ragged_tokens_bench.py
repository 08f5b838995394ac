#!/usr/bin/env python3
"""The visual-token generator on uniform and on ragged exemplar sets, one process, one handle: Engine.generate_tokens (1000 classes x
16 shots, the ViT-B/16 head: embed_dim 512, 4 aggregator layers, n_ctx 2) against Engine.generate_tokens_ragged on the same input
with all-16 shots, and on a ragged mix with the same number of rows (shots 1 .. 31).  The project's method: HIP events on the
launch stream, median of 20 calls after 5 (DESIGN.md section 4 holds the figures).

    python tools/ragged_tokens_bench.py [--classes 1000] [--shots 16] [--model ViT-B/16]
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ovmr_amd import modules, synth

ap = argparse.ArgumentParser()
ap.add_argument("--classes", type=int, default=1000)
ap.add_argument("--shots", type=int, default=16)
ap.add_argument("--model", default="ViT-B/16")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--calls", type=int, default=20)
a = ap.parse_args()
head = synth.SPECS[a.model]
# only the aggregator runs: tiny towers, the real head
spec = dataclasses.replace(synth.SPECS["tiny"], name="ragged_bench", embed_dim=head.embed_dim, transformer_width=head.embed_dim,
                           transformer_heads=head.embed_dim // 64, agg_layers=head.agg_layers)
sd = {k: torch.from_numpy(v) for k, v in synth.clip_state_dict(spec, 1).items()}
e = modules.CLIPModel(sd, spec).engine(2)
e.load_state_dict({}, {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, 2, 1).items()})
e._pl_loaded = True
e.finalize(8, 8, max(1024, a.classes))
C, S, D = a.classes, a.shots, spec.embed_dim
g = torch.Generator(device="cuda").manual_seed(1)
feats = torch.nn.functional.normalize(torch.randn(C * S, D, generator=g, device="cuda"), dim=-1).half()
mix = [1 + (7 * c) % (2 * S - 1) for c in range(C)]            # 1 .. 2 S - 1, mean S
step, i = (1 if sum(mix) < C * S else -1), 0
while sum(mix) != C * S:                                       # ... and the same number of rows as the uniform input
    if 1 <= mix[i % C] + step <= 2 * S - 1:
        mix[i % C] += step
    i += 1
assert min(mix) >= 1 and max(mix) <= 2 * S - 1 and 2 + max(mix) <= 128


def timed(fn):
    for _ in range(a.warmup):
        fn()
    ms = []
    for _ in range(a.calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return round(statistics.median(ms), 4)


out = {"classes": C, "shots": S, "rows": C * S, "dim": D, "agg_layers": spec.agg_layers, "mix_min_max": [min(mix), max(mix)]}
uniform = e.generate_tokens(feats.view(C, S, D))
assert torch.equal(uniform, e.generate_tokens_ragged(feats, [S] * C)), "all-equal shots differ from the uniform call"
out["uniform_ms"] = timed(lambda: e.generate_tokens(feats.view(C, S, D)))
out["ragged_all_equal_ms"] = timed(lambda: e.generate_tokens_ragged(feats, [S] * C))
out["ragged_mix_ms"] = timed(lambda: e.generate_tokens_ragged(feats, mix))
out["uniform_ms_again"] = timed(lambda: e.generate_tokens(feats.view(C, S, D)))
out["ragged_over_uniform"] = round(out["ragged_all_equal_ms"] / out["uniform_ms"], 4)
print(json.dumps(out))
