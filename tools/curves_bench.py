"""Times of the score-curve kernel (`eval_curves.hip`): ONE ovmr_eval_curves on a [256, C] output -- 1000 classes
fp32, 10 000 fp32, 21 841 fp16 -- at 256 and 4096 bins, beside the torch statement of the same step into a pre-allocated state,

    slot = torch.bucketize(out.float(), edges, right=True)                     # [B, C] int64, edges = linspace(lo, hi, bins + 1)
    state.view(-1).scatter_add_(0, ((class * 2 + own) * S + slot).view(-1), ones)   # B C same-or-not addresses

(the torch form buckets by pre-computed edges, so its cells can differ from the kernel's at an edge: it is here for its cost, not as a
reference), in the method of tools/retrieve_bench.py: HIP events on the launch stream around one call, 20 timed calls after 5, one
process, the forms ALTERNATING call by call.  Score patterns:

    softmax   rows of a softmax over C classes: nearly every negative of a class falls into ONE slot (the hot cell)
    logits    normal scores spread over the range: up to 64 distinct cells per (class, chunk of 64 rows)

    python tools/curves_bench.py            # one JSON line per case: median / min / max in microseconds
    python tools/curves_bench.py --pass     # also the test pass of bench.py's `--preset c3` shape (ViT-B/16, batch 256, 1000 classes,
                                            # 16 384 resident query images, EVAL_MODE fusion) with curves=256 against the same pass without:
                                            # milliseconds, median of 5 after a warm-up, the two taking turns
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


def timed_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def alternating(fns):
    """{name: (median, min, max)} of CALLS calls each, after WARMUP, the forms taking turns."""
    times = {n: [] for n in fns}
    for i in range(WARMUP + CALLS):
        for n, fn in fns.items():
            t = timed_us(fn)
            if i >= WARMUP:
                times[n].append(t)
    return {n: (round(statistics.median(t), 1), round(min(t), 1), round(max(t), 1)) for n, t in times.items()}


def torch_statement(out, labels, edges, state, classes, ones):
    C, S = state.shape[0], state.shape[2]
    slot = torch.bucketize(out.float(), edges, right=True)                       # [B, C] int64: 0 below lo ... bins + 1 at or above hi
    own = (labels.unsqueeze(1) == classes).long()
    state.view(-1).scatter_add_(0, ((classes * 2 + own) * S + slot).view(-1), ones)


def kernel_cases():
    rows = []
    for C, dtype in ((1000, torch.float32), (10000, torch.float32), (21841, torch.float16)):
        g = torch.Generator().manual_seed(C)
        labels = torch.randint(0, C, (B,), generator=g).cuda()
        classes = torch.arange(C, device="cuda").unsqueeze(0)
        ones = torch.ones(B * C, dtype=torch.int32, device="cuda")
        for name in ("softmax", "logits"):
            z = torch.randn((B, C), generator=g)
            out, (lo, hi) = (torch.softmax(z * 4, dim=1), (0.0, 1.0)) if name == "softmax" else (z * 10, (-40.0, 40.0))
            out = out.to(dtype).cuda()
            for bins in (256, 4096):
                state = torch.zeros((C, 2, bins + 3), dtype=torch.int32, device="cuda")
                other = torch.zeros_like(state)
                edges = torch.linspace(lo, hi, bins + 1, device="cuda")
                r = alternating({"eval_curves": lambda: runtime.eval_curves(out, labels, lo, hi, bins, state),
                                 "torch_scatter_add": lambda: torch_statement(out, labels, edges, other, classes, ones)})
                assert int(state.sum()) == int(other.sum()) == (WARMUP + CALLS) * B * C
                row = {"C": C, "B": B, "dtype": str(dtype)[6:], "pattern": name, "bins": bins,
                       "cells_hit": int((state != 0).sum()), "state_MB": round(state.numel() * 4 / 1e6, 1)}
                for n, (med, mn, mx) in r.items():
                    row[n + "_us"], row[n + "_min_us"], row[n + "_max_us"] = med, mn, mx
                rows.append(row)
                print(json.dumps(row), flush=True)
                del state, other
    return rows


def pass_case(C=1000, queries=16384, resident=4096, batch=256, bins=256):
    """The test pass of c3's shape on resident data (tools/all_modes_bench.py: CustomCLIP.forward_batches + Classification, EVAL_MODE
    fusion), with the score curves and without."""
    from ovmr_amd import modules, synth
    from ovmr_amd.evaluator import Classification
    spec = synth.SPECS["ViT-B/16"]
    D, R = spec.embed_dim, spec.image_resolution
    cm = modules.CLIPModel({k: torch.from_numpy(v) for k, v in synth.clip_state_dict(spec, 11, jitter=True).items()}, spec)
    cfg = modules.make_cfg(n_ctx=2, num_shots=16, output_dir="", test_batch_size=batch)
    pl = {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, 2, 11, True).items()}
    model = modules.CustomCLIP(cfg, torch.from_numpy(synth.class_token_ids(C, seed=9)), cm, prompt_learner_state=pl, reserve=(batch, 64, C),
                               stream_text=True)
    g = torch.Generator(device="cuda").manual_seed(8)
    unit = lambda: torch.nn.functional.normalize(torch.randn((C, D), generator=g, device="cuda"), dim=-1).half()     # noqa: E731
    model.mm_classifier, model.visual_classifer, model.zero_shot_classifier = unit(), unit(), unit()
    model.fusion_weight = torch.softmax(torch.randn((C, 3), generator=g, device="cuda"), -1)
    model.cfg.EVAL_MODE = "fusion"
    q = torch.randn((resident, 3, R, R), generator=g, device="cuda").half()
    labels = torch.randint(0, C, (resident,), generator=g, device="cuda")
    starts = [s for _ in range(max(1, queries // resident)) for s in range(0, resident, batch)]

    def one_pass(curves):
        ev = Classification(C, device="cuda", curves=curves)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.begin()
        for s, out in zip(starts, model.forward_batches((q[s:s + batch] for s in starts), stable_inputs=True)):
            ev.process(out, labels[s:s + batch])
        res = ev.evaluate(report=False)                      # the host reads the state once, and derives every figure
        dt = (time.perf_counter() - t0) * 1e3
        assert (curves is None) == ("mAP" not in res)
        return dt

    forms = {"plain_ms": None, "curves_ms": bins}
    times = {n: [] for n in forms}
    for i in range(6):
        for n, curves in forms.items():
            t = one_pass(curves)
            if i:
                times[n].append(t)
    row = {"pass": "CustomCLIP ViT-B/16 fusion", "C": C, "images": len(starts) * batch, "batch": batch, "bins": bins}
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
