"""Times of the bank audit (DESIGN.md section 4, row `neighbours_short`, and section 6, "Auditing the bank"), in the method of
tools/nearest_bench.py: HIP events on the launch stream around one call, 20 timed calls after 5, one process, the forms ALTERNATING call
by call; median with min and max, in microseconds.  D = 512.

(a) one class per query -- 1280 queries, classes of 16 and 64 rows, R = 16 000 and 640 000, k = 5 / 16 / 32 (capped at the class's rows):
      short          ovmr_neighbours_rows with max_range = the class's rows: one wave per query
      tiled          ovmr_nearest_rows restricted by `ranges`: the tiled launch pair, the code before the short kernel
      gather_topk    gather of every query's class rows + torch.bmm + ovmr_topk_rows
(b) the whole audit as CustomCLIP.audit_bank launches it, banks of 1000 x 16 and 10 000 x 64 synthetic rows, k = 5:
      in_class       every row against its own class without itself: ONE short launch over all R queries (and the same question on the
                     tiled pair, in batches, for comparison)
      out_of_class   every row against the bank without its class: the tiled pair in batches of 1024 queries
    The passes of the large bank take seconds: they are timed `--big-calls` times (default 3) after one.

    python tools/audit_bench.py [--skip-big]          # one JSON line per case
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ovmr_amd import runtime  # noqa: E402

D, B, CALLS, WARMUP = 512, 1280, 20, 5


def timed_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def alternating(fns, calls=CALLS, warmup=WARMUP):
    """{name: (median, min, max)} of `calls` calls each, after `warmup`, the forms taking turns."""
    times = {n: [] for n in fns}
    for i in range(warmup + calls):
        for n, fn in fns.items():
            t = timed_us(fn)
            if i >= warmup:
                times[n].append(t)
    return {n: (round(statistics.median(t), 1), round(min(t), 1), round(max(t), 1)) for n, t in times.items()}


def report(row, result):
    for n, (med, lo, hi) in result.items():
        row[n + "_us"], row[n + "_min_us"], row[n + "_max_us"] = med, lo, hi
    print(json.dumps(row), flush=True)
    return row


def features(R, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn((R, D), generator=g), dim=1).half().cuda(), g


def per_class(rows):
    for R in (16000, 640000):
        X, g = features(R, R)
        Q = torch.nn.functional.normalize(torch.randn((B, D), generator=g), dim=1).half().cuda()
        for n_rows in (16, 64):
            C = R // n_rows
            cls = torch.randint(0, C, (B,), generator=g).cuda()
            ranges = torch.stack([cls * n_rows, cls * n_rows + n_rows], 1).to(torch.int32)
            Xc = X.view(C, n_rows, D)
            for k in (5, 16, 32):
                kk = min(k, n_rows)
                if kk != k and kk in (5, 16):
                    continue                                      # (k = 32 on 16 rows is k = 16 again)
                r = alternating({"short": lambda: runtime.neighbour_rows(Q, X, kk, ranges, None, n_rows),
                                 "tiled": lambda: runtime.nearest_rows(Q, X, kk, ranges),
                                 "gather_topk": lambda: runtime.topk_rows(torch.bmm(Xc[cls], Q.unsqueeze(2)).squeeze(2), kk)})
                rows.append(report({"case": "per_class", "R": R, "B": B, "k": kk, "class_rows": n_rows}, r))
        del X


def whole_audit(rows, C, n_rows, calls, warmup, batch=1024, k=5):
    R = C * n_rows
    X, _ = features(R, C)
    r_all = torch.arange(R, device="cuda")
    own = torch.stack([r_all // n_rows * n_rows, r_all // n_rows * n_rows + n_rows], 1).to(torch.int32)
    me = torch.stack([r_all, r_all + 1], 1).to(torch.int32)
    out_v = torch.empty((R, k), dtype=torch.float32, device="cuda")
    out_i = torch.empty((R, k), dtype=torch.int32, device="cuda")

    def in_short():
        runtime.neighbour_rows(X, X, k, own, me, n_rows, out=(out_v, out_i))

    def in_tiled():
        for i in range(0, R, batch):
            runtime.neighbour_rows(X[i:i + batch], X, k, own[i:i + batch], me[i:i + batch], 0, out=(out_v[i:i + batch], out_i[i:i + batch]))

    def out_of_class():
        for i in range(0, R, batch):
            runtime.neighbour_rows(X[i:i + batch], X, k, None, own[i:i + batch], 0, out=(out_v[i:i + batch], out_i[i:i + batch]))

    r = alternating({"in_class_short": in_short, "in_class_tiled": in_tiled, "out_of_class": out_of_class}, calls, warmup)
    row = {"case": "audit", "classes": C, "class_rows": n_rows, "R": R, "k": k, "batch": batch, "calls": calls}
    row["total_us"] = round(r["in_class_short"][0] + r["out_of_class"][0], 1)
    rows.append(report(row, r))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-big", action="store_true", help="leave out the audit of the 10 000 x 64 bank")
    ap.add_argument("--big-calls", type=int, default=3)
    args = ap.parse_args(argv)
    runtime.load_library()
    rows = []
    per_class(rows)
    whole_audit(rows, 1000, 16, CALLS, WARMUP)
    if not args.skip_big:
        whole_audit(rows, 10000, 64, args.big_calls, 1)
    return rows


if __name__ == "__main__":
    main()
