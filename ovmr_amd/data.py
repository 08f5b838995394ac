"""Eval-set loader contract of the hot path on tensors already resident in HBM.

The reference's DataManager.eval_set_loader (Dassl RandomClassSampler, n_ins = NUM_SHOTS) yields
dict batches {"img": [Cb*S,3,R,R], "label": [Cb*S] int64} with S consecutive rows per class.  Image
decoding is out of scope; this loader only reproduces that layout over a pre-built tensor.
"""
from __future__ import annotations

from typing import Iterator, Optional

import torch


class ResidentEvalSet:
    """images [n_cls*S,3,R,R] (row c*S+s belongs to class_ids[c]); yields `classes_per_batch` classes at a
    time.  `presharded=True` tells CustomCLIP.forward_prompt that this rank owns every batch."""

    def __init__(self, images: torch.Tensor, class_ids: torch.Tensor, shots: int, classes_per_batch: int,
                 presharded: bool = False):
        assert images.shape[0] == class_ids.shape[0] * shots
        self.images, self.class_ids, self.shots = images, class_ids.to(torch.int64), shots
        self.cpb = max(1, classes_per_batch)
        self.presharded = presharded
        self._labels = self.class_ids.repeat_interleave(shots)

    def __len__(self) -> int:
        return (self.class_ids.shape[0] + self.cpb - 1) // self.cpb

    def __iter__(self) -> Iterator[dict]:
        step = self.cpb * self.shots
        for s in range(0, self.images.shape[0], step):
            yield {"img": self.images[s:s + step], "label": self._labels[s:s + step]}


class ResidentRaggedSet:
    """The ragged counterpart: images [R, 3, Res, Res] laid out class after class, `row_labels` [R] (host) the class of every row, a
    class owning as many rows as it has.  Yields whole classes, at most `batch_rows` rows at a time, with "shots" (host int64, one
    count per class of the batch); `.shots` is int32 [num_classes], the rows of every class of the vocabulary.  With world > 1 the
    set is class-sharded (`presharded`): a rank keeps the classes of its `shard_range`."""

    def __init__(self, images: torch.Tensor, row_labels, batch_rows: int, rank: int = 0, world: int = 1, num_classes: int = 0):
        from .shard import ragged_batches, shard_range, vocabulary_shots
        items = [(i, int(l)) for i, l in enumerate(torch.as_tensor(row_labels).tolist())]
        assert images.shape[0] == len(items)
        self.images, self.presharded = images, world > 1
        self.shots = vocabulary_shots(items, num_classes)
        if world > 1:
            lo, hi = shard_range(self.shots.shape[0], rank, world)
            items = [it for it in items if lo <= it[1] < hi]
        self.items = items
        self.spans = ragged_batches(items, batch_rows)

    def __len__(self) -> int:
        return len(self.spans)

    def __iter__(self) -> Iterator[dict]:
        for a, b, shots in self.spans:
            rows = torch.tensor([i for i, _ in self.items[a:b]], dtype=torch.long)
            yield {"img": self.images[rows.to(self.images.device)], "label": torch.tensor([l for _, l in self.items[a:b]], dtype=torch.long),
                   "shots": torch.tensor(shots, dtype=torch.long)}
