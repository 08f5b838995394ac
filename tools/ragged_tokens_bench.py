#!/usr/bin/env python3
"""The visual-token generator on uniform and on ragged exemplar sets, one process, one handle: Engine.generate_tokens (1000 classes x
16 shots, the ViT-B/16 head: embed_dim 512, 4 aggregator layers, n_ctx 2) against Engine.generate_tokens_ragged on the same input
with all-16 shots, and on a ragged mix with the same number of rows (shots 1 .. 31).  The project's method: HIP events on the
launch stream, median of 20 calls after 5 (DESIGN.md section 4 holds the figures).

--long adds the two mixes with classes beyond 126 images, on a second handle with option "agg_max_len" (the first keeps the default:
its three figures are those of a library that has no such option) -- 1000 classes x 16 with one class of 500, and 32 classes x 500 --
each beside the time Engine.encode_image of the real image tower (--model) takes for the SAME number of images, which is what an
exemplar set pays before its tokens are generated.

    python tools/ragged_tokens_bench.py [--classes 1000] [--shots 16] [--model ViT-B/16] [--long]
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
ap.add_argument("--long", action="store_true", help="also time the two long-class mixes and encode_image on as many images")
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
if a.long:
    LONG, BIG = 500, 32
    el = modules.CLIPModel(sd, spec).engine(2)
    el.load_state_dict({}, {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, 2, 1).items()})
    el._pl_loaded = True
    el.set_option("agg_max_len", 2 + LONG)
    el.finalize(8, 8, max(1024, a.classes))
    one_long = [S] * C
    one_long[C // 2] = LONG
    fl = torch.nn.functional.normalize(torch.randn(max(sum(one_long), BIG * LONG), D, generator=g, device="cuda"), dim=-1).half()
    short = el.generate_tokens_ragged(fl[:C * S], [S] * C)
    assert torch.equal(short, e.generate_tokens_ragged(fl[:C * S], [S] * C)), "short classes differ between the two handles"
    out["long_one_class_rows"] = sum(one_long)
    out["long_one_class_ms"] = timed(lambda: el.generate_tokens_ragged(fl[:sum(one_long)], one_long))
    out["long_all_rows"] = BIG * LONG
    out["long_all_ms"] = timed(lambda: el.generate_tokens(fl[:BIG * LONG].view(BIG, LONG, D)))
    out["long_all_ragged_ms"] = timed(lambda: el.generate_tokens_ragged(fl[:BIG * LONG], [LONG] * BIG))
    del el
    # the image tower of --model on as many images as each mix has rows, in loader batches of 512
    tower = modules.CLIPModel({k: torch.from_numpy(v) for k, v in synth.clip_state_dict(head, 1).items()}, head).engine(2)
    tower.load_state_dict({}, {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(head, 2, 1).items()})
    tower._pl_loaded = True
    tower.finalize(512, 8, 8)
    img = torch.randn(512, 3, head.image_resolution, head.image_resolution, generator=g, device="cuda").half()
    per_512 = timed(lambda: tower.encode_image(img, normalize=True))
    out["encode_image_512_ms"] = per_512
    out["encode_image_one_class_ms"] = round(per_512 * sum(one_long) / 512, 1)
    out["encode_image_all_ms"] = round(per_512 * BIG * LONG / 512, 1)
print(json.dumps(out))
