"""Times of the exact-ranks kernel (`eval_ranks.hip`): ONE ovmr_eval_ranks on a [256, C] batch of the kept scores
-- 1000 and 10 000 classes, fp32 and fp16 -- against an edge table of 16 distinct positive scores per class plus ONE class with 4000 (a
catch-all class: it is searched through L2, the others in LDS), beside the torch statement of the same step into a pre-allocated state,

    xt = out.float().t().contiguous()                                          # [C, B]: searchsorted wants the class outermost
    right, left = searchsorted(asc, xt, right=True), searchsorted(asc, xt)     # asc [C, max_edges]: each class's edges ascending, +inf padded
    cell = base + 2 * (count - right) + (right > left)                         # edges strictly above the score, tie or gap
    state.view(-1).scatter_add_(0, (own * plane + cell).view(-1), ones)        # B C same-or-not addresses

(finite scores only, where IEEE's order is the library's: the two states are asserted equal), in the method of tools/curves_bench.py: HIP
events on the launch stream around one call, 20 timed calls after 5, one process, the forms ALTERNATING call by call.  Score patterns:

    softmax   rows of a softmax over C classes: nearly every negative of a class lies below all its edges, in ONE cell
    logits    normal scores spread over the edges: up to 64 distinct cells per (class, chunk of 64 rows)

    python tools/ranks_bench.py            # one JSON line per case: median / min / max in microseconds, and `sweep_us`, the 64 batches of
                                           # a 16 384-image pass counted back to back (what evaluate() waits for)
    python tools/ranks_bench.py --pass     # also the test pass of bench.py's `--preset c3` shape (ViT-B/16, batch 256, 1000 classes,
                                           # 16 384 resident query images, EVAL_MODE fusion) with exact=True against the same pass without:
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
from curves_bench import CALLS, WARMUP, alternating, timed_us  # noqa: E402

B, N, PER_CLASS, CROWDED = 256, 16384, 16, 4000


def edge_table(C, pattern, g):
    """(edges fp32 [E] descending per class, estart int32 [C + 1]): PER_CLASS distinct values per class, CROWDED for class 0, drawn where
    the pattern's positives lie (exact in fp16: multiples of 2^-12 in [0, 1) for softmax, of 2^-6 in [-32, 32) for logits)."""
    counts = [CROWDED] + [PER_CLASS] * (C - 1)
    parts = []
    for n in counts:
        k = torch.randperm(4096, generator=g)[:n].float()
        v = k / 4096 if pattern == "softmax" else (k - 2048) / 64
        parts.append(torch.sort(v, descending=True)[0])
    estart = torch.zeros(C + 1, dtype=torch.int32)
    estart[1:] = torch.cumsum(torch.tensor(counts), 0)
    return torch.cat(parts), estart


def torch_statement(out, labels, asc, count, base, plane, state, classes, ones):
    xt = out.float().t().contiguous()
    right, left = torch.searchsorted(asc, xt, right=True), torch.searchsorted(asc, xt)
    cell = base + 2 * (count - right) + (right > left)
    own = (classes == labels.unsqueeze(0)).long()
    state.view(-1).scatter_add_(0, (own * plane + cell).view(-1), ones)


def kernel_cases():
    rows = []
    for C in (1000, 10000):
        for dtype in (torch.float32, torch.float16):
            g = torch.Generator().manual_seed(C)
            labels = torch.randint(0, C, (B,), generator=g).cuda()
            classes = torch.arange(C, device="cuda").unsqueeze(1)
            ones = torch.ones(B * C, dtype=torch.int32, device="cuda")
            for name in ("softmax", "logits"):
                z = torch.randn((B, C), generator=g)
                out = (torch.softmax(z * 4, dim=1) if name == "softmax" else z * 10).to(dtype).cuda()
                edges, estart = edge_table(C, name, g)
                E = edges.shape[0]
                asc = torch.full((C, CROWDED), float("inf"))
                for c in range(C):
                    asc[c, :estart[c + 1] - estart[c]] = edges[estart[c]:estart[c + 1]].flip(0)
                edges, estart, asc = edges.cuda(), estart.cuda(), asc.cuda()
                count = (estart[1:] - estart[:-1]).long().unsqueeze(1)
                base = (2 * estart[:-1].long() + torch.arange(C, device="cuda")).unsqueeze(1)
                plane = 2 * E + C
                state = torch.zeros((2, plane), dtype=torch.int32, device="cuda")
                other = torch.zeros_like(state)
                r = alternating({"eval_ranks": lambda: runtime.eval_ranks(out, labels, edges, estart, state, CROWDED),
                                 "torch_searchsorted": lambda: torch_statement(out, labels, asc, count, base, plane, other, classes, ones)})
                assert torch.equal(state, other) and int(state.sum()) == (WARMUP + CALLS) * B * C

                def sweep():
                    for _ in range(N // B):
                        runtime.eval_ranks(out, labels, edges, estart, state, CROWDED)
                sweeps = sorted(timed_us(sweep) for _ in range(5))
                row = {"C": C, "B": B, "dtype": str(dtype)[6:], "pattern": name, "E": E, "max_edges": CROWDED,
                       "cells_hit": int((state != 0).sum()), "state_MB": round(state.numel() * 4 / 1e6, 2), "sweep_us": round(sweeps[2], 1)}
                for n, (med, mn, mx) in r.items():
                    row[n + "_us"], row[n + "_min_us"], row[n + "_max_us"] = med, mn, mx
                rows.append(row)
                print(json.dumps(row), flush=True)
                del state, other, asc
    return rows


def pass_case(C=1000, queries=16384, resident=4096, batch=256):
    """The test pass of c3's shape on resident data (tools/curves_bench.py: pass_case), with the exact figures and without."""
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

    def one_pass(exact):
        ev = Classification(C, device="cuda", exact=exact)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.begin()
        for s, out in zip(starts, model.forward_batches((q[s:s + batch] for s in starts), stable_inputs=True)):
            ev.process(out, labels[s:s + batch])
        res = ev.evaluate(report=False)                      # the host builds the edges, the kernel counts, the host derives every figure
        dt = (time.perf_counter() - t0) * 1e3
        assert exact == ("exact_mAP" in res)
        return dt

    forms = {"plain_ms": False, "exact_ms": True}
    times = {n: [] for n in forms}
    for i in range(6):
        for n, exact in forms.items():
            t = one_pass(exact)
            if i:
                times[n].append(t)
    row = {"pass": "CustomCLIP ViT-B/16 fusion", "C": C, "images": len(starts) * batch, "batch": batch,
           "kept_MB": round(len(starts) * batch * C * 4 / 1e6, 1)}
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
