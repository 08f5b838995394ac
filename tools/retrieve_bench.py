"""Times of the search by class (`retrieve.hip`): ONE ovmr_retrieve_update on a [B, C] fp16 output, B = 256, at
C in {1000, 10000, 21841} and m in {5, 32}, beside ovmr_topk_rows at the same (B, C, k = m) -- what a second selection launch per batch
costs next to the first -- and beside the torch spelling of the same step,

    torch.cat([vals, out.t().float()], 1).topk(m)                  # vals fp32 [C, m]: the values carried from the batches before

in the method of tools/nearest_bench.py: HIP events on the launch stream around one call, 20 timed calls after 5, one process, the forms
ALTERNATING call by call.  Every update starts from the same state (restored outside the timed span).  Score patterns:

    random    random scores, empty state
    warm      random scores, the state of four earlier random batches (the steady state of a pass: few offers enter)
    rising    every column's scores rise along the batch: every offer enters its list, 256 serial insertions per class -- the worst case
    falling   every column's scores fall along the batch: nothing enters after the first chunk of 64 rows

    python tools/retrieve_bench.py            # one JSON line per case: median / min / max in microseconds
    python tools/retrieve_bench.py --pass     # also one retrieve pass against one predict pass (ViT-B/16 synthetic weights, zero-shot head,
                                              # 1000 classes, 4096 images in batches of 256): milliseconds, median of 5 after a warm-up
"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ovmr_amd import runtime  # noqa: E402

B, CALLS, WARMUP = 256, 20, 5


def timed_us(fn, before=None):
    if before is not None:
        before()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def alternating(fns, before=None):
    """{name: (median, min, max)} of CALLS calls each, after WARMUP, the forms taking turns; `before` runs untimed in front of every call."""
    times = {n: [] for n in fns}
    for i in range(WARMUP + CALLS):
        for n, fn in fns.items():
            t = timed_us(fn, before)
            if i >= WARMUP:
                times[n].append(t)
    return {n: (round(statistics.median(t), 1), round(min(t), 1), round(max(t), 1)) for n, t in times.items()}


def pattern(name, C, g):
    s = torch.randn((B, C), generator=g)
    if name in ("rising", "falling"):
        s = s.sort(dim=0, descending=name == "falling")[0]
    return s.half().cuda()


def kernel_cases():
    rows = []
    for C in (1000, 10000, 21841):
        g = torch.Generator().manual_seed(C)
        earlier = [torch.randn((B, C), generator=g).half().cuda() for _ in range(4)]
        for m in (5, 32):
            for name in ("random", "warm", "rising", "falling"):
                out = pattern(name, C, g)
                top = runtime.ColumnTopM(C, m)
                if name == "warm":
                    for i, e in enumerate(earlier):
                        top.update(e, i * B)
                start = top.state.clone()
                vals = top.finish()[0].clone()
                r = alternating({"update": lambda: top.update(out, 4 * B),
                                 "topk_rows": lambda: runtime.topk_rows(out, m),
                                 "torch_cat_topk": lambda: torch.cat([vals, out.t().float()], 1).topk(m)},
                                before=lambda: top.state.copy_(start))
                row = {"C": C, "B": B, "m": m, "pattern": name}
                for n, (med, lo, hi) in r.items():
                    row[n + "_us"], row[n + "_min_us"], row[n + "_max_us"] = med, lo, hi
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def pass_case(C=1000, n_images=4096, m=32, k=5):
    """One retrieve pass against one predict pass over the same resident batches (modules.ZeroshotCLIP on ViT-B/16 synthetic weights)."""
    from ovmr_amd import modules, synth
    spec = synth.SPECS["ViT-B/16"]
    clip = modules.CLIPModel({k_: torch.from_numpy(v) for k_, v in synth.clip_state_dict(spec, 11, jitter=True).items()}, spec)
    g = torch.Generator().manual_seed(5)
    ids = torch.zeros((C, spec.context_length), dtype=torch.long)
    ids[:, 0] = spec.vocab_size - 2
    ids[:, 1:8] = torch.randint(1, spec.vocab_size - 2, (C, 7), generator=g)
    ids[:, 8] = spec.vocab_size - 1                                                  # EOT: the largest id
    model = modules.ZeroshotCLIP(clip, ids, reserve=(B, 256, max(1024, C)))
    batches = [torch.randn((B, 3, spec.image_resolution, spec.image_resolution), generator=g).half().cuda() for _ in range(n_images // B)]

    def wall_ms(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    forms = {"predict_ms": lambda: [x for x in model.predict_topk_batches(iter(batches), k, stable_inputs=True)],
             "retrieve_ms": lambda: model.retrieve_batches(iter(batches), m, stable_inputs=True).finish(),
             "retrieve_within_top_ms": lambda: model.retrieve_batches(iter(batches), m, within_top=k, stable_inputs=True).finish()}
    times = {n: [] for n in forms}
    for i in range(6):
        for n, fn in forms.items():
            t = wall_ms(fn)
            if i:
                times[n].append(t)
    row = {"pass": "ZeroshotCLIP ViT-B/16", "C": C, "images": n_images, "batch": B, "m": m, "k": k}
    for n, t in times.items():
        row[n], row[n[:-3] + "_min_ms"], row[n[:-3] + "_max_ms"] = round(statistics.median(t), 2), round(min(t), 2), round(max(t), 2)
    print(json.dumps(row), flush=True)
    return row


def main():
    runtime.load_library()
    rows = kernel_cases()
    if "--pass" in sys.argv:
        rows.append(pass_case())
    return rows


if __name__ == "__main__":
    main()
