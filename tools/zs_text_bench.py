"""Wall time of building the ZeroshotCLIP2 text classifier (ovmr_encode_text_ensemble) on ViT-B/16 synthetic weights.

    python tools/zs_text_bench.py [--classes 1000 21841] [--templates 8] [--reps 5]

Token ids: SOT, 5-14 random tokens (the length range of the IMAGENET_TEMPLATES_SELECT prompts of typical class names), EOT; each template
gets its own exact length, as Engine.encode_text_ensemble computes it for host ids.  Prints one JSON line per class count: median wall
time of the call (host enqueue to stream synchronisation, the ids already on the device) over --reps runs after one warm-up.  Run it under
`rocprofv3 --kernel-trace --stats` for the share of each kernel.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ovmr_amd import synth  # noqa: E402
from ovmr_amd.runtime import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, nargs="+", default=[1000, 21841])
    ap.add_argument("--templates", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    spec = synth.SPECS["ViT-B/16"]
    e = Engine(spec, 2)
    e.load_state_dict({k: torch.from_numpy(v) for k, v in synth.clip_state_dict(spec, 11, jitter=True).items()},
                      {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, 2, 11, True).items()})
    e.finalize(256, 256, 1024)                                   # the runner's reserve (cli.main, test batch 256)
    rng = np.random.default_rng(0)
    for C in a.classes:
        T = a.templates
        ids = np.zeros((T, C, 77), dtype=np.int64)
        n = rng.integers(5, 15, (T, C))
        for t in range(T):
            for c in range(C):
                ids[t, c, 0], ids[t, c, 1 + n[t, c]] = synth.SOT_ID, synth.EOT_ID
                ids[t, c, 1:1 + n[t, c]] = rng.integers(1, synth.SOT_ID, n[t, c])
        sl = (ids.argmax(-1).max(1) + 1).tolist()
        dev = torch.from_numpy(ids).cuda()
        e.encode_text_ensemble(dev, seq_lens=sl)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            e.encode_text_ensemble(dev, seq_lens=sl)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        print(json.dumps({"classes": C, "templates": T, "seq_lens": sl, "prompts": T * C, "token_rows": C * sum(sl),
                          "wall_ms_median": round(1e3 * float(np.median(ts)), 3), "wall_ms_all": [round(1e3 * x, 3) for x in ts]}), flush=True)


if __name__ == "__main__":
    main()
