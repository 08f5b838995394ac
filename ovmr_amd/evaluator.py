"""On-device classification evaluator.

Arithmetic of Dassl's `Classification` evaluator (Dassl.pytorch/dassl/evaluation/evaluator.py:50-138): top-1 accuracy,
error rate, macro-F1 and per-class accuracy / F1, accumulated as three histograms on the GPU by ONE launch per batch of
the library's own row-argmax-and-count kernel (`ovmr_eval_counts`, csrc/fusion_head.hip: the cross-validation step's
counting, on the [B, C] outputs) -- the reference does `.item()` and `.cpu().numpy()` per batch (:59-67), i.e. one host
sync per batch of 256 images; here the host reads 3C + 1 integers once, in evaluate().

Detail mode (`per_class=True` and / or `confusion=True`: the reference's TEST.PER_CLASS_RESULT / TEST.COMPUTE_CMAT, evaluator.py:38-40,
69-73, 140-171) keeps everything an integer counter on the device as well: ONE `ovmr_eval_detail` launch per batch (csrc/eval_detail.hip)
does the counting above plus the per-class matches and the [C, C] confusion counts; evaluate() prints the reference's `=> per-class
result` block and writes `cmat.pt`, the array sklearn's confusion_matrix(normalize="true") returns.  With both off nothing changes.

Score curves (`curves=BINS`; no counterpart in the reference): one more integer state beside the histograms, int32 [C, 2, BINS + 3] -- per
class the distribution of the scores of its own rows (plane 1) and of everybody else's (plane 0) over `score_range`, by the slot function
of include/ovmr_hip_curves.h -- filled by ONE `ovmr_eval_curves` launch per batch (csrc/eval_curves.hip).  evaluate() derives every
class's average precision, AUROC and best-F1 operating point from it, adds `mAP` and `mean_auroc` to the results and two lines to the
result block, and writes `curves_per_class.csv` and `score_hist.pt`.  With `curves=None` nothing of this is allocated, launched, printed
or written.

Outputs that live on the GPU go through the kernel and nothing else: without libovmr_hip.so `process` raises.  Host
tensors (an evaluator built with device="cpu": host-side callers, the CPU tests of evaluate()'s arithmetic) are counted
on the host.
"""
from __future__ import annotations

import os
from collections import OrderedDict
from typing import Optional, Sequence

import torch


CURVE_COLUMNS = ["label", "classname", "positives", "negatives", "ap", "auroc", "best_f1", "slot", "threshold", "precision", "recall"]


def curve_slots(x: torch.Tensor, lo: float, hi: float, bins: int) -> torch.Tensor:
    """The slot function of include/ovmr_hip_curves.h in torch float32 on the host: x (any shape) -> int64 slots in [0, bins + 3).  The
    subtraction and the product are two float32 operations (each rounded once, nothing fused); the comparisons are IEEE's, which order
    everything but NaN as the library's key does (-0.0 == +0.0, a denormal is not flushed)."""
    from .runtime import curve_scale
    flo, fhi, scale = (float(v) for v in curve_scale(lo, hi, bins, "curve_slots"))
    x = x.detach().float().cpu()
    t = (x - flo) * scale
    inside = (x >= flo) & (x < fhi)                                       # (False for a NaN)
    j = torch.floor(torch.where(inside, t, torch.zeros_like(t))).long().clamp_(max=bins - 1)
    slot = torch.where(inside, 1 + j, torch.zeros_like(j))
    slot = torch.where(x >= fhi, torch.full_like(slot, bins + 1), slot)
    return torch.where(x != x, torch.full_like(slot, bins + 2), slot)


def curve_figures(hist, lo: float, hi: float, bins: int) -> dict:
    """hist: int64 [C, 2, bins + 3] (plane 0 negatives, plane 1 positives of every class, by slot) -> per-class float64 numpy arrays, the
    slots walked from the highest down: a cut AT slot s calls everything in the slots >= s a hit.
      positives P, negatives N (int64);
      ap      sum over slots of (positives in the slot / P) x precision at that cut   (sklearn's average_precision_score with the slot as
              the score); NaN where P == 0;
      auroc   sum over slots of pos_s x (negatives below s + neg_s / 2) / (P N)       (roc_auc_score, ties at half); NaN where P N == 0;
      best_f1, slot, precision, recall: the cut of the largest F1 = 2 tp / (tp + fp + P), ties to the HIGHER slot; NaN / -1 where P == 0;
      threshold: that slot's NOMINAL lower edge lo + (slot - 1)(hi - lo) / bins in fp64 (-inf for slot 0, which admits everything; NaN for
              the NaN slot).  Nominal: the slot function, in fp32, is what decides which scores the cut admits."""
    import numpy as np
    h = np.asarray(hist, dtype=np.int64)
    C, S = h.shape[0], h.shape[2]
    assert h.shape == (C, 2, bins + 3), (h.shape, bins)
    neg, pos = h[:, 0].astype(np.float64), h[:, 1].astype(np.float64)
    P, N = h[:, 1].sum(axis=1), h[:, 0].sum(axis=1)
    Pf, Nf = P.astype(np.float64)[:, None], N.astype(np.float64)[:, None]
    tp = np.cumsum(pos[:, ::-1], axis=1)[:, ::-1]                          # positives in the slots >= s
    fp = np.cumsum(neg[:, ::-1], axis=1)[:, ::-1]
    below = np.cumsum(neg, axis=1) - neg                                   # negatives in the slots < s
    with np.errstate(all="ignore"):
        prec = np.where(tp + fp > 0, tp / (tp + fp), 0.0)
        ap = np.where(P > 0, (pos / Pf * prec).sum(axis=1), np.nan)
        auroc = np.where((P > 0) & (N > 0), (pos * (below + neg / 2)).sum(axis=1) / (Pf * Nf)[:, 0], np.nan)
        f1 = np.where(Pf > 0, 2 * tp / (tp + fp + Pf), 0.0)
        slot = S - 1 - np.argmax(f1[:, ::-1], axis=1)                      # (argmax: the first maximum = the highest slot)
        rows = np.arange(C)
        have = P > 0
        rec = tp[rows, slot] / Pf[:, 0]
    lo, hi = float(lo), float(hi)
    thr = lo + (slot - 1).astype(np.float64) * (hi - lo) / bins
    thr = np.where(slot == 0, -np.inf, np.where(slot == S - 1, np.nan, thr))
    return dict(positives=P, negatives=N, ap=ap, auroc=auroc, best_f1=np.where(have, f1[rows, slot], np.nan), slot=np.where(have, slot, -1),
                threshold=np.where(have, thr, np.nan), precision=np.where(have, prec[rows, slot], np.nan), recall=np.where(have, rec, np.nan))


class Classification:
    def __init__(self, num_classes: int, classnames: Optional[Sequence[str]] = None, device="cuda", per_class: bool = False,
                 confusion: bool = False, curves: Optional[int] = None, score_range=(0.0, 1.0)):
        self.num_classes = num_classes
        self.curve_bins, self.score_range = None, None
        if curves is not None:
            from .runtime import MAX_BINS, curve_scale
            if isinstance(curves, bool) or not isinstance(curves, int) or not 1 <= curves <= MAX_BINS:
                raise ValueError(f"Classification: curves must be None or a number of bins in [1, {MAX_BINS}], got {curves!r}")
            if not isinstance(score_range, (tuple, list)) or len(score_range) != 2:
                raise ValueError(f"Classification: score_range must be a pair (lo, hi), got {score_range!r}")
            flo, fhi, _ = curve_scale(score_range[0], score_range[1], curves, "Classification")
            self.curve_bins, self.score_range = int(curves), (float(flo), float(fhi))      # (the range as the fp32 values that decide)
        self.per_class, self.confusion = bool(per_class), bool(confusion)
        self.classnames = list(classnames) if classnames is not None else [str(i) for i in range(num_classes)]
        self.device = torch.device(device)
        self.reset()

    def reset(self):
        # int32 [3][C] = tp, n_pred, n_label, + one slot counting rows whose label is outside [0, C) (include/ovmr_hip.h: ovmr_eval_counts)
        self._counts = torch.zeros(3 * self.num_classes + 1, dtype=torch.int32, device=self.device)
        self._topk = None                            # the `topk` of this pass, set by begin() or by its first process()
        self._hits = None                            # int32 [1], topk > 1: rows whose label is among their k best columns
        # detail mode, allocated by begin() / the first process() of the pass (the matches depend on its topk)
        self._class_hits = None                      # int32 [C], per_class and topk > 1: such rows per label (at topk == 1 that is tp)
        self._cmat = None                            # int32 [C, C], confusion: rows per (label, top-1 prediction)
        self.confusion_counts = None                 # int64 [C, C] on the host, set by evaluate()
        self._curves = None                          # int32 [C, 2, bins + 3], curves=: allocated by begin() (include/ovmr_hip_curves.h)
        self.score_hist = None                       # int64 [C, 2, bins + 3] on the host, and
        self.curves = None                           # curve_figures() of it, both set by evaluate()

    def begin(self, topk: int = 1):
        """Allocates the state of a pass that uses `topk`, without a batch: what the first process() of a pass does by itself.  A pass
        sharded over ranks calls it up front on every rank (trainer._EvalTrainer.test), so that a rank without a single batch enters
        `all_reduce` with the tensors its peers hold."""
        C = self.num_classes
        topk = int(topk)
        if not 1 <= topk <= min(32, C):
            raise ValueError(f"topk {topk} outside [1, min(32, {C} classes)]")
        if self._topk is not None:
            raise ValueError(f"begin(topk={topk}) in a pass that began already (topk={self._topk}): reset() starts the next")
        self._topk = topk
        if topk > 1:
            self._hits = torch.zeros(1, dtype=torch.int32, device=self.device)
            if self.per_class:
                self._class_hits = torch.zeros(C, dtype=torch.int32, device=self.device)
        if self.confusion:
            self._cmat = torch.zeros((C, C), dtype=torch.int32, device=self.device)
        if self.curve_bins is not None:
            self._curves = torch.zeros((C, 2, self.curve_bins + 3), dtype=torch.int32, device=self.device)

    @staticmethod
    def all_reduce(evaluators: Sequence["Classification"], dist) -> None:
        """Sums the state of the evaluators of ONE pass over the process group `dist` (torch.distributed), in place: afterwards every rank
        holds the job's counters.  The small counters of all of them travel in one all-reduce, each confusion matrix in one of its own
        (shard.all_reduce_eval_state).  Every evaluator has begun its pass (begin(), or a first process()), with the same topk and the
        same flags on every rank: the collectives' shapes then do not depend on what a rank counted.  A score-curve state travels like a
        confusion matrix, in an all-reduce of its own."""
        from .shard import all_reduce_eval_state
        small, cmats = [], []
        for ev in evaluators:
            if ev._topk is None:
                raise RuntimeError("Classification.all_reduce before begin(): a rank without a batch would enter the collective with fewer "
                                   "tensors than its peers")
            small += [t for t in (ev._counts, ev._hits, ev._class_hits) if t is not None]
            if ev._cmat is not None:
                cmats.append(ev._cmat)
            if ev._curves is not None:
                cmats.append(ev._curves)
        all_reduce_eval_state(small, cmats, dist)

    @torch.no_grad()
    def process(self, mo: torch.Tensor, gt: torch.Tensor, topk: int = 1):
        """mo: [B, C] model output (fp32 probabilities of CustomCLIP.forward, or fp16 zero-shot logits), gt: [B] labels
        (evaluator.py:50-67).  One kernel launch on the current stream, no host synchronisation.  topk > 1 (:56-58): a row counts as
        correct when its label is among its k best columns (ovmr_topk_rows: one more launch, hits accumulate on the device); the
        histograms -- macro-F1, the per-class tables -- keep coming from the top-1 prediction, the reference's pred[:, 0] (:64-65).
        One pass uses one topk."""
        C = self.num_classes
        if mo.dim() != 2 or mo.shape[1] != C or gt.shape[0] != mo.shape[0]:
            raise ValueError(f"Classification.process: mo must be [B, {C}] ({C} classes) and gt [B], got mo {list(mo.shape)} and "
                             f"gt {list(gt.shape)}")
        if self._topk is None:
            self.begin(topk)
        elif int(topk) != self._topk:
            raise ValueError(f"process(topk={topk}) in a pass that began with topk={self._topk}: one pass uses one topk (reset() starts the next)")
        topk = self._topk
        if self.device.type == "cpu":
            pred, ok = self._process_host(mo, gt)
            gt = gt.long()
            if self._curves is not None:
                self._curves_host(mo, gt, ok)
            if topk > 1:
                order = torch.sort(mo.float(), dim=1, descending=True, stable=True)[1][:, :topk]     # the library's total order
                hit = (order == gt.unsqueeze(1)).any(dim=1)
                self._hits += int(hit.sum())
                if self._class_hits is not None:
                    self._class_hits += torch.bincount(gt[ok & hit], minlength=C).int()
            if self._cmat is not None:
                self._cmat.index_put_((gt[ok], pred[ok]), torch.ones(int(ok.sum()), dtype=torch.int32), accumulate=True)
            return
        from . import runtime
        lib = runtime.load_library()                                      # raises without the HIP library: no fallback for device tensors
        mo = mo.to(self.device)
        if mo.dtype not in (torch.float16, torch.float32):
            mo = mo.float()
        if mo.stride(1) != 1:
            mo = mo.contiguous()
        gt = gt.to(self.device, non_blocking=True)
        if gt.dtype != torch.int64 or not gt.is_contiguous():
            gt = gt.long().contiguous()
        if self._curves is not None:                                      # ONE launch: every score into its class's two histograms
            runtime.eval_curves(mo, gt, self.score_range[0], self.score_range[1], self.curve_bins, self._curves)
        if self.per_class or self.confusion:                              # ONE launch: counts, hits, per-class matches, confusion counts
            if mo.shape[0]:
                runtime.eval_detail(mo, gt, topk, self._counts, self._hits, self._class_hits, self._cmat)
            return
        rc = lib.ovmr_eval_counts(runtime._ptr(mo), runtime.F32 if mo.dtype == torch.float32 else runtime.F16, mo.stride(0),
                                  runtime._ptr(gt), mo.shape[0], C, runtime._ptr(self._counts), runtime._stream())
        if rc != 0:
            raise runtime.OvmrError(f"ovmr_eval_counts failed with {rc}")
        if topk > 1 and mo.shape[0]:
            runtime.topk_rows(mo, topk, gt, self._hits)

    def _process_host(self, mo, gt):
        """The same three histograms for host tensors (mo.max(1)[1]: lowest column on ties); returns (pred, rows with a label in [0, C))."""
        C = self.num_classes
        pred = mo.float().argmax(dim=1)
        gt = gt.long()
        bad = (gt < 0) | (gt >= C)
        ok = ~bad
        c = self._counts
        c[3 * C] += int(bad.sum())
        c[2 * C:3 * C] += torch.bincount(gt[ok], minlength=C).int()
        c[C:2 * C] += torch.bincount(pred[ok], minlength=C).int()
        c[:C] += torch.bincount(gt[ok & (pred == gt)], minlength=C).int()
        return pred, ok

    def _curves_host(self, mo, gt, ok):
        """ovmr_eval_curves for host tensors: the same cells, by curve_slots (gt int64, ok: rows with a label in [0, C))."""
        C, S = self.num_classes, self.curve_bins + 3
        slot = curve_slots(mo, self.score_range[0], self.score_range[1], self.curve_bins)[ok]        # [n, C]
        own = (gt[ok].unsqueeze(1) == torch.arange(C).unsqueeze(0)).long()
        cell = (torch.arange(C).unsqueeze(0) * 2 + own) * S + slot
        self._curves += torch.bincount(cell.reshape(-1), minlength=C * 2 * S).int().view(C, 2, S)

    def counts(self):
        """(tp, n_pred, n_label) as int64 host tensors [C]; raises if a label outside [0, C) was seen."""
        c = self._counts.cpu().long()
        C = self.num_classes
        if int(c[3 * C]):
            raise ValueError(f"{int(c[3 * C])} test label(s) outside [0, {C})")
        return c[:C], c[C:2 * C], c[2 * C:3 * C]

    def evaluate(self, output_dir: Optional[str] = None, report: bool = True) -> "OrderedDict[str, float]":
        """report=False: the figures alone -- nothing is printed and no file is written (ranks > 0 of a sharded pass, which hold the
        job's counters after all_reduce and leave the reporting to rank 0)."""
        say = print if report else (lambda *a, **k: None)
        if not report:
            output_dir = None
        tp_i, n_pred_i, n_label_i = self.counts()
        tp, n_pred, n_label = tp_i.double(), n_pred_i.double(), n_label_i.double()
        total = float(n_label.sum())
        correct = int(tp.sum()) if self._hits is None else int(self._hits.cpu()[0])        # evaluator.py:56-60
        acc = 100.0 * correct / max(total, 1.0)
        precision = torch.where(n_pred > 0, tp / n_pred.clamp(min=1), torch.zeros_like(tp))
        recall = torch.where(n_label > 0, tp / n_label.clamp(min=1), torch.zeros_like(tp))
        f1 = torch.where(precision + recall > 0, 2 * precision * recall / (precision + recall).clamp(min=1e-300),
                         torch.zeros_like(tp))
        present = n_label > 0                                             # f1_score(labels=np.unique(y_true)), evaluator.py:104-123
        macro_f1 = 100.0 * float(f1[present].mean()) if bool(present.any()) else 0.0
        res = OrderedDict(accuracy=acc, error_rate=100.0 - acc, macro_f1=macro_f1)
        self.per_class_accuracy = (100.0 * recall).tolist()
        self.per_class_f1 = (100.0 * f1).tolist()
        say("=> result\n"
              f"* total: {int(total):,}\n* correct: {correct:,}\n* accuracy: {acc:.1f}%\n"
              f"* error: {100.0 - acc:.1f}%\n* macro_f1: {macro_f1:.1f}%")       # the format parse_test_res.py greps for
        if self.curve_bins is not None:
            self._evaluate_curves(res, output_dir, say)
        if output_dir:                                                    # evaluator.py:84-113 (csv module formats)
            import csv
            os.makedirs(output_dir, exist_ok=True)
            labels = [i for i in range(self.num_classes) if n_label[i] > 0]
            with open(os.path.join(output_dir, "acc_per_class.csv"), "w", newline="") as f:
                w = csv.writer(f, delimiter=",")
                w.writerow(["Label", "Acc"])
                for key in sorted(str(i) for i in labels):                  # the reference sorts the labels as strings
                    w.writerow([key, self.per_class_accuracy[int(key)]])
            with open(os.path.join(output_dir, "f1_per_class.csv"), "w", newline="") as f:
                w = csv.writer(f, delimiter=",")
                w.writerow(["Label", "F1"])
                for item_id, i in enumerate(labels):
                    w.writerow([item_id, self.per_class_f1[i]])
        if self.per_class:                                                # evaluator.py:140-163, its format byte for byte
            import numpy as np
            matches = tp_i if self._class_hits is None else self._class_hits.cpu().long()      # top-k matches when topk > 1 (:56-58, 69-73)
            say("=> per-class result")
            accs = []
            for label in range(self.num_classes):
                total_c, correct_c = int(n_label_i[label]), int(matches[label])
                if total_c == 0:                                          # _per_class_res has a key per label that occurred
                    continue
                acc_c = 100.0 * correct_c / total_c
                accs.append(acc_c)
                say(f"* class: {label} ({self.classnames[label]})\ttotal: {total_c:,}\tcorrect: {correct_c:,}\tacc: {acc_c:.1f}%")
            mean_acc = float(np.mean(accs)) if accs else 0.0
            say(f"* average: {mean_acc:.1f}%")
            res["perclass_accuracy"] = mean_acc
        if self.confusion:                                                # evaluator.py:165-171
            C = self.num_classes
            cm = self._cmat.cpu().long() if self._cmat is not None else torch.zeros((C, C), dtype=torch.int64)
            self.confusion_counts = cm
            if output_dir:
                import numpy as np
                os.makedirs(output_dir, exist_ok=True)
                # sklearn.metrics.confusion_matrix(y_true, y_pred, normalize="true") from the counts: the classes that occur as a label
                # or as a prediction, in increasing order; every row over its sum, 0 / 0 -> 0.  The same int64 / int64 division and
                # nan_to_num as sklearn's own, so the array is its array bit for bit
                present = ((n_label_i > 0) | (n_pred_i > 0)).numpy()
                sub = cm.numpy()[present][:, present]
                with np.errstate(all="ignore"):
                    sub = np.nan_to_num(sub / sub.sum(axis=1, keepdims=True))
                save_path = os.path.join(output_dir, "cmat.pt")
                torch.save(sub, save_path)
                print(f"Confusion matrix is saved to {save_path}")
        return res

    def _evaluate_curves(self, res, output_dir, say):
        """The score-curve part of evaluate(): figures from the int64 state on the host, two more lines of the result block, two files."""
        import numpy as np
        C, bins = self.num_classes, self.curve_bins
        lo, hi = self.score_range
        hist = self._curves.cpu().long() if self._curves is not None else torch.zeros((C, 2, bins + 3), dtype=torch.int64)
        self.score_hist = hist
        fig = self.curves = curve_figures(hist.numpy(), lo, hi, bins)
        ranked, separated = fig["positives"] > 0, (fig["positives"] > 0) & (fig["negatives"] > 0)
        res["mAP"] = 100.0 * float(fig["ap"][ranked].mean()) if ranked.any() else 0.0
        res["mean_auroc"] = float(fig["auroc"][separated].mean()) if separated.any() else 0.0
        say(f"* mAP: {res['mAP']:.1f}%\n* mean_auroc: {res['mean_auroc']:.4f}")
        if output_dir:
            import csv
            os.makedirs(output_dir, exist_ok=True)

            def cell(v):                                                  # a figure a class does not have is an empty field
                return "" if v != v else (int(v) if isinstance(v, (int, np.integer)) else float(v))
            with open(os.path.join(output_dir, "curves_per_class.csv"), "w", newline="") as f:
                w = csv.writer(f, delimiter=",")
                w.writerow(CURVE_COLUMNS)
                for c in range(C):
                    have = bool(ranked[c])
                    w.writerow([c, self.classnames[c], int(fig["positives"][c]), int(fig["negatives"][c]), cell(fig["ap"][c]), cell(fig["auroc"][c]),
                                cell(fig["best_f1"][c]), int(fig["slot"][c]) if have else "",
                                (repr(float(fig["threshold"][c])) if have else ""), cell(fig["precision"][c]), cell(fig["recall"][c])])
            torch.save({"hist": hist, "lo": lo, "hi": hi, "bins": bins}, os.path.join(output_dir, "score_hist.pt"))
