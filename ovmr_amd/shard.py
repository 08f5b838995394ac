"""Class sharding for multi-GPU classifier generation (one process per GPU, torch.distributed;
backend "nccl" is RCCL over xGMI on ROCm, "gloo" in the CPU tests).

The reference has no distributed path; the path shards naturally because classes are
independent until the cross-validation step:
  * every rank encodes the exemplars of its own classes and produces their mm / vision / text
    classifier rows and visual tokens;
  * ONE all-gather of the packed rows [bound, 3*D + n_ctx*D + 2] fp16 (mm | vision | text | visual tokens | label bits)
    assembles the classifier matrix (5 MB in total at 1000 classes: latency bound, far below the ~153 GB/s of one xGMI
    link); the per-rank block size `bound` follows from C, the world size and the loader contract, so no size exchange
    precedes it;
  * every rank runs the argmax counting for its own exemplar rows against all classes and ONE
    all-reduce sums the int32 [3,2,C] counters (n_pred[c] receives votes from other ranks' rows).

The test pass shards by BATCHES (`shard_test_batches`): rank r evaluates a contiguous range of the batches of the one-process pass --
same item order, same batch boundaries, so every output row is the one-process row bit for bit (a batch's size selects kernels and
the head's implementation; an item split would move the boundaries) -- and counts them into its own evaluator state, integer
counters whose sum over the ranks is the job's (`all_reduce_eval_state`: ONE all-reduce for the small counters of every evaluator
of the pass, one per confusion matrix).
"""
from __future__ import annotations

from typing import List, Tuple

import torch


def shard_range(n: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous, balanced split of n units: ranks < n % world get one extra unit."""
    base, rem = divmod(n, world)
    start = rank * base + min(rank, rem)
    return start, start + base + (1 if rank < rem else 0)


def shard_test_batches(n_items: int, batch_size: int, rank: int, world: int) -> Tuple[Tuple[int, int], Tuple[int, int]]:
    """The split of a test pass: `n_items` items in batches of `batch_size` (the last one ragged), as one process walks them ->
    ((first item, end item), (first batch, end batch)) of `rank`: the contiguous `shard_range` of the BATCHES, and the items those
    batches hold.  A rank beyond the number of batches gets an empty range of both."""
    n_batches = -(-n_items // batch_size)
    first, end = shard_range(n_batches, rank, world)
    return (min(first * batch_size, n_items), min(end * batch_size, n_items)), (first, end)


def keep_batch_shard(items: list, batch_size: int, batch_shard, ragged: bool = False):
    """What a loader's `batch_shard=(rank, world)` keeps of `items` -> (items of the rank's batches, (rank, world), [first, end) of its
    batches); batch_shard None: (items, None, None).  Refused with a ragged exemplar set, whose batches hold whole classes and are
    sharded by class."""
    if batch_shard is None:
        return items, None, None
    if ragged:
        raise ValueError("batch_shard= shards a test pass by batches: not with ragged=True (an exemplar set is sharded by class: rank=, world=)")
    rank, world = (int(v) for v in batch_shard)
    if not 0 <= rank < world:
        raise ValueError(f"batch_shard=({rank}, {world}): the rank lies in [0, world)")
    (a, b), span = shard_test_batches(len(items), batch_size, rank, world)
    return items[a:b], (rank, world), span


def shard_batches(num_batches: int, rank: int, world: int) -> List[int]:
    """Round-robin assignment used by CustomCLIP.forward_prompt (batch i belongs to rank i % world)."""
    return [i for i in range(num_batches) if i % world == rank]


def local_class_bound(num_classes: int, world: int, presharded: bool, classes_per_batch: int) -> int:
    """Upper bound of the classes ONE rank produces, computed from values every rank knows (no communication).
    presharded loaders own a contiguous `shard_range` of the classes; otherwise batch i belongs to rank i % world and a
    batch holds at most `classes_per_batch` = TEST.BATCH_SIZE // NUM_SHOTS classes, which bounds a rank's
    share by C / world + 2 * classes_per_batch for any batch size up to that."""
    if presharded:
        return -(-num_classes // world)
    return -(-num_classes // world) + 2 * max(1, classes_per_batch)


def ragged_batches(items, batch_size: int) -> List[Tuple[int, int, List[int]]]:
    """The batches of a ragged exemplar set: `items` [(path, label)] laid out class after class (cli.layout_exemplars_ragged) ->
    [(start, end, shots of the batch's classes)], whole classes per batch, as many as fit `batch_size` rows.  A class with more rows
    than a batch holds is refused here, before anything is decoded."""
    runs: List[Tuple[int, int, int]] = []                      # (label, start, end) of every run of equal labels
    for i, it in enumerate(items):
        if runs and runs[-1][0] == it[1]:
            runs[-1] = (it[1], runs[-1][1], i + 1)
        else:
            runs.append((it[1], i, i + 1))
    if len({r[0] for r in runs}) != len(runs):
        raise ValueError("a ragged exemplar set lists every class's rows consecutively (cli.layout_exemplars_ragged)")
    out: List[Tuple[int, int, List[int]]] = []
    for label, a, b in runs:
        if b - a > batch_size:
            raise ValueError(f"class {label} has {b - a} exemplar rows, more than one batch of DATALOADER.TEST.BATCH_SIZE = {batch_size} holds")
        if out and b - out[-1][0] <= batch_size:
            out[-1] = (out[-1][0], b, out[-1][2] + [b - a])
        else:
            out.append((a, b, [b - a]))
    return out


def vocabulary_shots(items, num_classes: int) -> torch.Tensor:
    """int32 [num_classes]: the exemplar rows of every class of the WHOLE item list (what a ragged loader publishes as `.shots`: every
    rank knows it from the list, so the F1 preference's n_label needs no collective)."""
    n = torch.zeros(max(num_classes, 1 + max((it[1] for it in items), default=-1)), dtype=torch.int32)
    for it in items:
        n[it[1]] += 1
    return n


def _staged(t: torch.Tensor, dist) -> torch.Tensor:
    """gloo moves host memory: stage device tensors through the CPU (CPU tests, or several ranks sharing one GPU)."""
    return t.cpu() if dist.get_backend() == "gloo" and t.is_cuda else t


def pack_block(rows: torch.Tensor, labels: torch.Tensor, bound: int) -> torch.Tensor:
    """One rank's contribution to the all-gather: [bound, K + 2] fp16 = its rows, the int32 label of each row carried in two
    extra fp16 columns (bit pattern, not value), padding rows labelled -1."""
    n, K = rows.shape
    if n > bound:
        raise RuntimeError(f"this rank produced {n} classes, more than the bound {bound} every rank agreed on: the eval-set "
                           "loader yields more than TEST.BATCH_SIZE // NUM_SHOTS classes per batch")
    assert rows.dtype == torch.float16
    lab = torch.full((bound,), -1, dtype=torch.int32, device=rows.device)
    lab[:n] = labels.to(torch.int32)
    block = torch.zeros((bound, K + 2), dtype=torch.float16, device=rows.device)
    block[:n, :K] = rows
    block[:, K:] = lab.view(torch.float16).reshape(bound, 2)
    return block


def all_gather_rows(rows: torch.Tensor, labels: torch.Tensor, bound: int, dist) -> Tuple[torch.Tensor, torch.Tensor]:
    """ONE all-gather of a ragged set of fp16 rows.  rows [n_local, K] fp16, labels [n_local] (class ids), n_local <= bound
    (`local_class_bound`, identical on every rank).  Every rank contributes one `pack_block`.
    Returns (all_rows [world * bound, K], all_labels [world * bound] int32 with -1 on padding rows), rank-major."""
    K = rows.shape[1]
    world = dist.get_world_size()
    block = _staged(pack_block(rows, labels, bound), dist)
    out = torch.empty((world * bound, K + 2), dtype=torch.float16, device=block.device)
    dist.all_gather_into_tensor(out, block)
    out = out.to(rows.device)
    return out[:, :K], out[:, K:].contiguous().view(torch.int32).reshape(-1)


def all_gather_block(block: torch.Tensor, dist) -> torch.Tensor:
    """ONE all-gather of every rank's `pack_block`-format block [bound, K + 2] fp16 (Engine.pack_rows builds it in one launch) ->
    [world * bound, K + 2], rank-major, on the block's device."""
    b = _staged(block, dist)
    out = torch.empty((dist.get_world_size() * b.shape[0], b.shape[1]), dtype=torch.float16, device=b.device)
    dist.all_gather_into_tensor(out, b)
    return out.to(block.device)


def all_gather_retrieve_state(state: torch.Tensor, dist) -> torch.Tensor:
    """ONE all-gather of every rank's runtime.ColumnTopM.state, int64 [C, m] (opaque, byte-copyable: include/ovmr_hip_retrieve.h) ->
    [world, C, m] on the state's device, rank-major.  A rank without a batch sends its empty (all-zero) state."""
    s = _staged(state.contiguous(), dist)
    world = dist.get_world_size()
    out = torch.empty((world * s.shape[0], s.shape[1]), dtype=torch.int64, device=s.device)      # (gloo takes the concatenated form only)
    dist.all_gather_into_tensor(out, s)
    return out.view(world, s.shape[0], s.shape[1]).to(state.device)


def all_gather_positives(scores: torch.Tensor, labels: torch.Tensor, dist) -> Tuple[torch.Tensor, torch.Tensor]:
    """The positives of an exact test pass (evaluator.Classification.count_ranks) from every rank: scores fp32 [n] and labels int64 [n]
    on the host, n the rank's own count -> (scores [sum n], labels [sum n]) on the host, rank-major.  Ragged: ONE all-gather of the
    lengths, then ONE of the pairs padded to the longest rank, each as int64 [max n, 2] = (the score's bits, the label) so that a NaN or a
    -0.0 arrives as it left.  A rank without a batch sends nothing but padding."""
    world, backend = dist.get_world_size(), dist.get_backend()
    dev = torch.device("cpu") if backend == "gloo" else torch.device("cuda", torch.cuda.current_device())
    n = torch.tensor([scores.numel()], dtype=torch.int64, device=dev)
    lengths = torch.empty(world, dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(lengths, n)
    lengths = lengths.cpu().tolist()
    longest = max(max(lengths), 1)
    block = torch.zeros((longest, 2), dtype=torch.int64)
    block[:scores.numel(), 0] = scores.float().contiguous().view(torch.int32).long()
    block[:scores.numel(), 1] = labels.long()
    block = block.to(dev)
    out = torch.empty((world * longest, 2), dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(out, block)
    out = out.cpu().view(world, longest, 2)
    pairs = torch.cat([out[r, :lengths[r]] for r in range(world)])
    return pairs[:, 0].int().view(torch.float32), pairs[:, 1].contiguous()


def all_reduce_counts(counts: torch.Tensor, dist) -> torch.Tensor:
    """ONE all-reduce (sum) of the int32 [3, 2, C] argmax counters."""
    c = _staged(counts, dist)
    dist.all_reduce(c)
    return c.to(counts.device)


def all_reduce_eval_state(small: List[torch.Tensor], cmats: List[torch.Tensor], dist) -> None:
    """Sums the evaluator state of a test pass over the ranks, IN PLACE.  `small`: the int32 counter vectors of every evaluator of the
    pass (evaluator.Classification: _counts, _hits, _class_hits), concatenated into ONE all-reduce and split back; `cmats`: the int32
    [C, C] confusion counts, one all-reduce each (a matrix is not copied into a concatenation).  Every rank passes the same number of
    tensors with the same shapes, whatever it counted (Classification.begin); int32 sums over ranks are the one-process int32 sums."""
    if small:
        flat = _staged(torch.cat([t.reshape(-1) for t in small]), dist)
        dist.all_reduce(flat)
        for t, part in zip(small, flat.split([t.numel() for t in small])):
            t.copy_(part.reshape(t.shape))
    for m in cmats:
        c = _staged(m, dist)
        dist.all_reduce(c)
        if c is not m:
            m.copy_(c)
