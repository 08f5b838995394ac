"""Times of the evaluator's launches (DESIGN.md section 4, rows `eval_detail` and `topk_rows`): ovmr_eval_detail beside the launches it
replaces -- ovmr_eval_counts alone at k = 1, ovmr_eval_counts + ovmr_topk_rows at k > 1 -- and torch.topk, on [256, C] fp32 outputs.
HIP events on the launch stream around one call (or the pair), median of 20 calls after a warm-up of 5, all in one process.

    python tools/eval_detail_bench.py            # C = 1000 and 21 841; random labels and one (label, pred) cell; with and without cmat
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ovmr_amd import runtime  # noqa: E402

B, CALLS, WARMUP = 256, 20, 5


def median_us(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return round(statistics.median(times), 1)


def main():
    lib = runtime.load_library()
    P, S = runtime._ptr, runtime._stream
    rows = []
    for C in (1000, 21841):
        g = torch.Generator().manual_seed(C)
        mo = torch.softmax(torch.randn((B, C), generator=g) * 3, dim=1).cuda()
        pred = mo.argmax(1)
        for labels_kind in ("random", "one_cell"):
            if labels_kind == "one_cell":                                # every row predicts class 7 and carries label 7
                mo = mo.clone()
                mo[:, 7] = 2.0
                lab = torch.full((B,), 7, dtype=torch.int64, device="cuda")
            else:
                lab = torch.where(torch.rand(B, generator=g).cuda() < 0.7, pred, torch.randint(0, C, (B,), generator=g).cuda()).contiguous()
            counts = torch.zeros(3 * C + 1, dtype=torch.int32, device="cuda")
            hits = torch.zeros(1, dtype=torch.int32, device="cuda")
            class_hits = torch.zeros(C, dtype=torch.int32, device="cuda")
            idx = torch.zeros((B, 32), dtype=torch.int32, device="cuda")
            for k in (1, 5):
                def old():
                    lib.ovmr_eval_counts(P(mo), 1, C, P(lab), B, C, P(counts), S())
                    if k > 1:
                        lib.ovmr_topk_rows(P(mo), 1, C, B, C, k, None, P(idx), P(lab), P(hits), S())
                row = {"C": C, "labels": labels_kind, "k": k, "replaced_us": median_us(old)}
                if k > 1:
                    row["eval_counts_us"] = median_us(lambda: lib.ovmr_eval_counts(P(mo), 1, C, P(lab), B, C, P(counts), S()))
                    row["topk_rows_us"] = median_us(lambda: lib.ovmr_topk_rows(P(mo), 1, C, B, C, k, None, P(idx), P(lab), P(hits), S()))
                    row["torch_topk_us"] = median_us(lambda: torch.topk(mo, k, dim=1))
                for with_cmat in (True, False):
                    cmat = torch.zeros((C, C), dtype=torch.int32, device="cuda") if with_cmat else None
                    h, ch = (hits, class_hits) if k > 1 else (None, None)
                    row["detail_cmat_us" if with_cmat else "detail_no_cmat_us"] = median_us(
                        lambda: lib.ovmr_eval_detail(P(mo), 1, C, P(lab), B, C, k, P(counts), P(h), P(ch), P(cmat), S()))
                    del cmat
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


if __name__ == "__main__":
    main()
