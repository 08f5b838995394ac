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

Exact ranking figures (`exact=True`; no counterpart in the reference): the figures of the binned scores above are not those a paper reports.
For one class every exact figure depends only on where each negative falls relative to the class's own positive scores, and those are known
when the pass ends.  So `process()` keeps every batch's outputs on their device (under `exact_max_bytes`), and at the end of the pass
`count_ranks()` builds per class the table of its distinct positive scores (`rank_edges`) and counts every kept batch against it -- ONE
`ovmr_eval_ranks` launch per batch (csrc/eval_ranks.hip, include/ovmr_hip_ranks.h) into an int32 [2, 2E + C] state -- and frees the scores.
evaluate() derives every class's average precision, AUROC and best-F1 operating point from the counts (`rank_figures`: sklearn's figures on
the raw scores), adds `exact_mAP` and `exact_mean_auroc` to the results and two lines to the result block, and writes `ranks_per_class.csv`
and `rank_state.pt`.  With `exact=False` nothing of this is kept, launched, printed or written.

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


RANK_COLUMNS = ["label", "classname", "positives", "negatives", "ap", "auroc", "best_f1", "threshold", "precision", "recall"]


def rank_keys(x):
    """The value part of the library's selection key (csrc/eval_common.h: topk_key) of fp32 values, as numpy uint32 of the same shape:
    x above y in the library's order <=> key(x) > key(y); every NaN is one key, the largest; -0.0 and +0.0 share theirs; a denormal keeps
    its own."""
    import numpy as np
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).copy()
    u[u == 0x80000000] = 0
    u = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    u[np.isnan(x)] = 0xFFFFFFFF
    return u


def _key_values(k):
    """rank_keys inverted: the canonical fp32 of every key (one NaN, +0.0 for either zero)."""
    import numpy as np
    k = np.asarray(k, dtype=np.uint32)
    u = np.where(k & 0x80000000, k ^ np.uint32(0x80000000), ~k).astype(np.uint32)
    u[k == 0xFFFFFFFF] = 0x7FC00000
    return u.view(np.float32)


def rank_edges(pos_scores, pos_labels, C: int):
    """The edge table of include/ovmr_hip_ranks.h from the positives of a pass: pos_scores [n] (any float dtype; the score every image
    gave its own class) and pos_labels [n] -> (edges fp32 [E], estart int32 [C + 1]) on the host.  Scores are canonicalised first (-0
    becomes +0, any NaN the one NaN 0x7FC00000); class c's edges are its distinct scores, strictly descending in the library's value order
    (NaN first).  Labels outside [0, C) have no class and are left out.  Deterministic in the MULTISET of (score, label) pairs: their
    order, and which rank sent which, do not matter."""
    import numpy as np
    s = torch.as_tensor(pos_scores).detach().float().cpu().reshape(-1).numpy()
    y = torch.as_tensor(pos_labels).detach().cpu().reshape(-1).numpy().astype(np.int64)
    if s.shape != y.shape:
        raise ValueError(f"rank_edges: pos_scores and pos_labels must be of one length, got {s.shape[0]} and {y.shape[0]}")
    ok = (y >= 0) & (y < C)
    # ascending in (label, 2^32 - 1 - key) = by class, then descending by value; np.unique leaves each (class, value) once
    pairs = np.unique((y[ok].astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - rank_keys(s[ok]).astype(np.uint64)))
    cls = (pairs >> np.uint64(32)).astype(np.int64)
    edges = _key_values((np.uint64(0xFFFFFFFF) - (pairs & np.uint64(0xFFFFFFFF))).astype(np.uint32))
    estart = np.zeros(C + 1, dtype=np.int64)
    estart[1:] = np.cumsum(np.bincount(cls, minlength=C))
    if estart[-1] >= 2 ** 31:
        raise ValueError(f"rank_edges: {int(estart[-1])} edges do not fit estart's int32")
    return torch.from_numpy(edges.copy()), torch.from_numpy(estart.astype(np.int32))


def rank_cells(mo, edges, estart, max_edges: Optional[int] = None) -> torch.Tensor:
    """The cell rule of include/ovmr_hip_ranks.h on the host: mo [B, C] (any float dtype), edges fp32 [E], estart int32 [C + 1] -> int64
    [B, C], the cell of mo[b, c] WITHIN class c (add 2 estart[c] + c for its place in a plane): with k the number of the class's edges
    strictly above the score in the library's value order, 2 k + 1 where edge k equals the score, else 2 k.  estart is clamped as the
    kernel clamps it, and a class is searched against its first min(E_c, max_edges) edges (None: all of them)."""
    import numpy as np
    x = rank_keys(torch.as_tensor(mo).detach().float().cpu().numpy())
    B, C = x.shape
    ek = rank_keys(torch.as_tensor(edges).detach().float().cpu().numpy())
    es = torch.as_tensor(estart).cpu().numpy().astype(np.int64)
    E = ek.shape[0]
    cells = np.zeros((B, C), dtype=np.int64)
    for c in range(C):
        lo = min(max(int(es[c]), 0), E)
        hi = min(max(int(es[c + 1]), lo), E)
        n = hi - lo if max_edges is None else min(hi - lo, int(max_edges))
        if n == 0:
            continue
        asc = ek[lo:lo + n][::-1]                                            # ascending keys
        above = n - np.searchsorted(asc, x[:, c], side="right")              # edges strictly above the score
        tied = np.searchsorted(asc, x[:, c], side="right") > np.searchsorted(asc, x[:, c], side="left")
        cells[:, c] = 2 * above + tied
    return torch.from_numpy(cells)


def rank_count(state: torch.Tensor, mo, gt, edges, estart, max_edges: Optional[int] = None) -> None:
    """ovmr_eval_ranks for host tensors: adds one batch to state int32 [2, 2E + C] in place, by rank_cells."""
    B, C = mo.shape
    gt = torch.as_tensor(gt).long().cpu()
    ok = (gt >= 0) & (gt < C)
    es = torch.as_tensor(estart).long().cpu()
    E = int(torch.as_tensor(edges).shape[0])
    base = 2 * es[:C].clamp(0, E) + torch.arange(C)
    cell = (rank_cells(mo, edges, estart, max_edges) + base.unsqueeze(0))[ok]
    own = (gt[ok].unsqueeze(1) == torch.arange(C).unsqueeze(0)).long()
    flat = (own * (2 * E + C) + cell).reshape(-1)
    state += torch.bincount(flat, minlength=2 * (2 * E + C)).to(state.dtype).view(2, 2 * E + C)


def rank_figures(state, edges, estart) -> dict:
    """state: integer [2, 2E + C] (plane 0 negatives, plane 1 positives; class c's 2 E_c + 1 cells from 2 estart[c] + c), edges fp32 [E],
    estart int32 [C + 1] -> per-class numpy arrays, computed from int64 counts in fp64.  With pos_k and neq_k the counts tied with edge k
    of a class (edges descending: k = 0 is the highest score), ngap_k the negatives in the gap above it, P and N the class's totals:
      TP_k = cumsum(pos), FP_k = cumsum(neq + ngap): what a cut AT edge k admits;
      ap      sum_k pos_k / P x TP_k / (TP_k + FP_k)            (sklearn's average_precision_score on the raw scores); NaN where P == 0;
      auroc   sum_k pos_k x ((N - FP_k) + neq_k / 2) / (P N)    (roc_auc_score, ties at half); NaN where P N == 0;
      best_f1 max_k 2 TP_k / (2 TP_k + FP_k + P - TP_k), ties to the HIGHER threshold, with threshold = that edge itself (a real score),
              precision and recall of the cut; NaN where P == 0.
    A positive in an even cell (a gap) raises: every positive IS an edge, so the kept scores or labels changed under the evaluator."""
    import numpy as np
    st = torch.as_tensor(state).cpu().numpy().astype(np.int64)
    ed = torch.as_tensor(edges).cpu().numpy().astype(np.float32)
    es = torch.as_tensor(estart).cpu().numpy().astype(np.int64)
    C, E = es.shape[0] - 1, ed.shape[0]
    if st.shape != (2, 2 * E + C):
        raise ValueError(f"rank_figures: state must be of shape [2, {2 * E + C}] for {E} edges and {C} classes, got {list(st.shape)}")
    out = {k: np.full(C, np.nan) for k in ("ap", "auroc", "best_f1", "threshold", "precision", "recall")}
    P, N = np.zeros(C, dtype=np.int64), np.zeros(C, dtype=np.int64)
    for c in range(C):
        n, base = int(es[c + 1] - es[c]), 2 * int(es[c]) + c
        neg, own = st[0, base:base + 2 * n + 1], st[1, base:base + 2 * n + 1]
        if own[0::2].any():
            raise ValueError(f"rank_figures: class {c} holds {int(own[0::2].sum())} positive(s) between its edges: the kept scores or labels "
                             "changed after the edges were built")
        pos, neq, ngap = own[1::2].astype(np.float64), neg[1::2].astype(np.float64), neg[0:2 * n:2].astype(np.float64)
        P[c], N[c] = own.sum(), neg.sum()
        if P[c] == 0:
            continue
        p, q = float(P[c]), float(N[c])
        tp, fp = np.cumsum(pos), np.cumsum(neq + ngap)
        prec = tp / (tp + fp)                                                # (tp >= 1 at every edge: an edge is a positive's score)
        out["ap"][c] = float((pos / p * prec).sum())
        if N[c] > 0:
            out["auroc"][c] = float((pos * ((q - fp) + neq / 2)).sum() / (p * q))
        f1 = 2 * tp / (2 * tp + fp + p - tp)
        k = int(np.argmax(f1))                                               # (the first maximum: the highest threshold)
        out["best_f1"][c], out["precision"][c], out["recall"][c] = f1[k], prec[k], tp[k] / p
        out["threshold"][c] = ed[int(es[c]) + k]
    return dict(positives=P, negatives=N, **out)


class Classification:
    def __init__(self, num_classes: int, classnames: Optional[Sequence[str]] = None, device="cuda", per_class: bool = False,
                 confusion: bool = False, curves: Optional[int] = None, score_range=(0.0, 1.0), exact: bool = False,
                 exact_max_bytes: int = 16 << 30):
        self.num_classes = num_classes
        if not isinstance(exact, bool):
            raise ValueError(f"Classification: exact must be True or False, got {exact!r}")
        if isinstance(exact_max_bytes, bool) or not isinstance(exact_max_bytes, int) or exact_max_bytes < 0:
            raise ValueError(f"Classification: exact_max_bytes must be a number of bytes >= 0, got {exact_max_bytes!r}")
        self.exact, self.exact_max_bytes = exact, int(exact_max_bytes)
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
        self._kept = []                              # exact=: (outputs [B, C] as they arrived, labels int64 [B]) of every batch of the pass
        self._kept_bytes = 0                         # bytes of the kept outputs, held under exact_max_bytes
        self._rank = None                            # (edges fp32 [E], estart int32 [C + 1], state int32 [2, 2E + C]) once counted
        self.rank_state = None                       # the same three on the host, state as int64, and
        self.ranks = None                            # rank_figures() of them, both set by evaluate()

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
        confusion matrix, in an all-reduce of its own.  An exact evaluator (exact=True) then counts its kept scores (count_ranks): one
        all-gather of the lengths and one of the padded (score, label) pairs of the positives, every rank builds the same edges and counts
        its own batches, and one all-reduce sums the int32 state."""
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
        for ev in evaluators:
            if ev.exact:
                ev.count_ranks(dist)

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
            if self.exact:
                self._keep(mo, gt)
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
        if self.exact:
            self._keep(mo, gt)
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

    def _keep(self, mo, gt):
        """exact=: keeps the batch's outputs in the dtype they arrived in, on their device, with the labels, until the pass ends -- a copy
        of their own, since a model may write its next batch where this one stands.  The batch that would pass exact_max_bytes raises."""
        if self._rank is not None:
            raise ValueError("Classification.process after the exact figures of the pass were counted: reset() starts the next")
        if mo.dtype not in (torch.float16, torch.float32):
            mo = mo.float()
        need = mo.shape[0] * mo.shape[1] * mo.element_size()
        if self._kept_bytes + need > self.exact_max_bytes:
            raise ValueError(f"Classification(exact=True): keeping this batch's {list(mo.shape)} {mo.dtype} outputs takes the score store to "
                             f"{self._kept_bytes + need:,} bytes, beyond exact_max_bytes = {self.exact_max_bytes:,}")
        self._kept_bytes += need
        self._kept.append((mo.detach().clone(memory_format=torch.contiguous_format), gt.detach().clone()))

    def count_ranks(self, dist=None) -> None:
        """exact=: the end of the pass.  Takes the positives of the kept batches (the score every image gave its own class), builds the
        edge table (rank_edges), counts every kept batch into the state of include/ovmr_hip_ranks.h -- ONE ovmr_eval_ranks launch per
        batch on the device, rank_count on the host -- and frees the kept scores.  With a process group `dist` the positives of all ranks
        are gathered first, so that every rank builds the same edges, and the int32 state is summed over the ranks afterwards."""
        if not self.exact or self._rank is not None:
            return
        C, dev = self.num_classes, self.device
        scores, labels = [], []
        for mo, gt in self._kept:
            ok = (gt >= 0) & (gt < C)
            at = torch.where(ok, gt, torch.zeros_like(gt))
            scores.append(mo.gather(1, at.unsqueeze(1)).squeeze(1)[ok].float())
            labels.append(gt[ok])
        s = torch.cat(scores).cpu() if scores else torch.zeros(0, dtype=torch.float32)
        y = torch.cat(labels).cpu() if labels else torch.zeros(0, dtype=torch.int64)
        if dist is not None:
            from .shard import all_gather_positives
            s, y = all_gather_positives(s, y, dist)
        edges, estart = rank_edges(s, y, C)
        E = edges.shape[0]
        max_edges = int((estart[1:] - estart[:-1]).max())
        edges, estart = edges.to(dev), estart.to(dev)
        state = torch.zeros((2, 2 * E + C), dtype=torch.int32, device=dev)
        for mo, gt in self._kept:
            if dev.type == "cpu":
                rank_count(state, mo, gt, edges, estart, max_edges)
            else:
                from . import runtime
                runtime.eval_ranks(mo, gt, edges, estart, state, max_edges)
        if dist is not None:
            from .shard import all_reduce_eval_state
            all_reduce_eval_state([], [state], dist)
        self._kept, self._kept_bytes = [], 0                              # the score store is freed
        self._rank = (edges, estart, state)

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
        if self.exact:
            self._evaluate_ranks(res, output_dir, say)
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

    def _evaluate_ranks(self, res, output_dir, say):
        """The exact part of evaluate(): counts the kept scores unless all_reduce did, figures from the int64 state on the host, two more
        lines of the result block, two files."""
        import numpy as np
        self.count_ranks()
        edges, estart, state = (t.cpu() for t in self._rank)
        state = state.long()
        self.rank_state = (edges, estart, state)
        fig = self.ranks = rank_figures(state, edges, estart)
        ranked, separated = fig["positives"] > 0, (fig["positives"] > 0) & (fig["negatives"] > 0)
        res["exact_mAP"] = 100.0 * float(fig["ap"][ranked].mean()) if ranked.any() else 0.0
        res["exact_mean_auroc"] = float(fig["auroc"][separated].mean()) if separated.any() else 0.0
        say(f"* exact_mAP: {res['exact_mAP']:.1f}%\n* exact_mean_auroc: {res['exact_mean_auroc']:.4f}")
        if output_dir:
            import csv
            os.makedirs(output_dir, exist_ok=True)

            def cell(v):                                                  # a figure a class does not have is an empty field
                return "" if v != v else float(v)
            with open(os.path.join(output_dir, "ranks_per_class.csv"), "w", newline="") as f:
                w = csv.writer(f, delimiter=",")
                w.writerow(RANK_COLUMNS)
                for c in range(self.num_classes):
                    w.writerow([c, self.classnames[c], int(fig["positives"][c]), int(fig["negatives"][c]), cell(fig["ap"][c]), cell(fig["auroc"][c]),
                                cell(fig["best_f1"][c]), (repr(float(fig["threshold"][c])) if ranked[c] else ""), cell(fig["precision"][c]),
                                cell(fig["recall"][c])])
            torch.save({"edges": edges, "estart": estart, "state": state, "classnames": list(self.classnames)},
                       os.path.join(output_dir, "rank_state.pt"))
