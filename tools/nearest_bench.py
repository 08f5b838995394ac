"""Times of the nearest-exemplar search (DESIGN.md section 4, row `nearest_rows`): ovmr_nearest_rows beside what the library offered
before it -- torch.matmul in fp16, which writes the [B, R] score matrix, followed by ovmr_topk_rows -- in the method of
tools/eval_detail_bench.py: HIP events on the launch stream around one call, 20 timed calls after 5, one process, the two forms ALTERNATING
call by call.  D = 512, k = 5 and 32, R = 16 000 and 640 000 (the 10 000 x 64 vocabulary):

    whole bank     B = 256 queries
    per class      1280 queries (256 images x 5 predicted classes), each restricted to one class of 16 / 64 rows (R / 1000 and R / 10 000
                   rows per class); the composition gathers every query's class rows, multiplies them (torch.bmm) and ranks the [1280, n]
                   result with ovmr_topk_rows (k capped at the class's rows)

    python tools/nearest_bench.py            # one JSON line per case: median / min / max in microseconds
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ovmr_amd import runtime  # noqa: E402

D, B, CALLS, WARMUP = 512, 256, 20, 5


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


def main():
    runtime.load_library()
    rows = []
    for R in (16000, 640000):
        g = torch.Generator().manual_seed(R)
        X = torch.nn.functional.normalize(torch.randn((R, D), generator=g), dim=1).half().cuda()
        Q = torch.nn.functional.normalize(torch.randn((B, D), generator=g), dim=1).half().cuda()
        for k in (5, 32):
            r = alternating({"fused": lambda: runtime.nearest_rows(Q, X, k),
                             "matmul_topk": lambda: runtime.topk_rows(torch.matmul(Q, X.t()), k)})
            row = {"R": R, "B": B, "k": k, "ranges": None}
            for n, (med, lo, hi) in r.items():
                row[n + "_us"], row[n + "_min_us"], row[n + "_max_us"] = med, lo, hi
            rows.append(row)
            print(json.dumps(row), flush=True)
        for n_rows in (16, 64):
            C = R // n_rows
            cls = torch.randint(0, C, (B * 5,), generator=g).cuda()
            Q5 = Q.repeat_interleave(5, 0)
            ranges = torch.stack([cls * n_rows, cls * n_rows + n_rows], 1).to(torch.int32)
            Xc = X.view(C, n_rows, D)
            for k in (5, 32):
                kk = min(k, n_rows)
                r = alternating({"fused": lambda: runtime.nearest_rows(Q5, X, kk, ranges),
                                 "matmul_topk": lambda: runtime.topk_rows(torch.bmm(Xc[cls], Q5.unsqueeze(2)).squeeze(2), kk)})
                row = {"R": R, "B": B * 5, "k": kk, "ranges": n_rows}
                for n, (med, lo, hi) in r.items():
                    row[n + "_us"], row[n + "_min_us"], row[n + "_max_us"] = med, lo, hi
                rows.append(row)
                print(json.dumps(row), flush=True)
        del X
    return rows


if __name__ == "__main__":
    main()
