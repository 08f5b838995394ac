"""The test pass sharded over ranks, on the host: the split (shard.shard_test_batches through the loaders' batch_shard=), the evaluator's
begin() / all_reduce() under gloo, and _EvalTrainer.test() under gloo with a stand-in model -- every counter, result, printed block and
written file of a W-rank pass against the one-process pass of the same code, by equality.  Every spawned group has a 30 s timeout: a
collective that a rank does not enter ends the test instead of hanging it.

The evaluator case is the issue's -- 5 classes, 11 rows in batches of 4 -- which is THREE batches (4 + 4 + 3): worlds 2 and 3 split them
2 + 1 and 1 + 1 + 1, and world 4 is added so that a rank (rank 3) holds no batch at all.  The trainer case has 7 rows in batches of 4, two
batches, so that world 3 leaves rank 2 without one."""
import datetime
import io
import os
import socket
import sys
from contextlib import redirect_stdout
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import REPO

GROUP_TIMEOUT = datetime.timedelta(seconds=30)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _open_group(rank, world, port):
    sys.path.insert(0, REPO)
    torch.set_num_threads(1)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=GROUP_TIMEOUT)


def _count_all_reduces():
    calls = []
    real = dist.all_reduce

    def counted(t, *a, **k):
        calls.append(tuple(t.shape))
        return real(t, *a, **k)

    dist.all_reduce = counted
    return calls


# ----------------------------------------------------------------------------- 1. the split
def test_shard_spans_concatenate_to_the_one_process_loader():
    from ovmr_amd import cli
    from ovmr_amd.loader import PipelinedFolderLoader
    from ovmr_amd.shard import shard_range, shard_test_batches
    for n in range(24):
        items = [(f"{i}.jpg", i % 3) for i in range(n)]
        for bs in range(1, 6):
            one = cli.FolderLoader(items, bs, 16)
            assert one.batch_shard is None and one.batch_range is None
            want = [one.items[a:b] for a, b, _ in one.spans]                     # the batches of the one-process pass
            for world in range(1, 6):
                got, ranges = [], []
                for rank in range(world):
                    ld = cli.FolderLoader(items, bs, 16, batch_shard=(rank, world))
                    assert ld.batch_shard == (rank, world) and not ld.presharded and len(ld) == len(ld.spans)
                    got += [ld.items[a:b] for a, b, _ in ld.spans]
                    ranges.append(tuple(ld.batch_range))
                    assert tuple(ld.batch_range) == shard_range(len(want), rank, world) and len(ld) == ranges[-1][1] - ranges[-1][0]
                    (lo, hi), span = shard_test_batches(n, bs, rank, world)
                    assert span == ranges[-1] and ld.items == items[lo:hi]
                    if (n + bs + world) % 7 == 0:                                 # (a sample: the pipelined loader states the same spans)
                        pl = PipelinedFolderLoader(items, bs, 16, batch_shard=(rank, world), device="cpu")
                        assert (pl.items, pl.spans, pl.batch_shard, tuple(pl.batch_range)) == (ld.items, ld.spans, (rank, world), ranges[-1])
                assert got == want, (n, bs, world)
                assert ranges[0][0] == 0 and ranges[-1][1] == len(want)
                assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))      # contiguous, in rank order
                sizes = [b - a for a, b in ranges]
                assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)


def test_empty_shard_iterates_and_ragged_is_refused():
    from ovmr_amd import cli
    from ovmr_amd.loader import PipelinedFolderLoader
    items = [(f"{i}.jpg", 0) for i in range(7)]
    for make in (lambda **kw: cli.FolderLoader(items, 4, 16, **kw), lambda **kw: PipelinedFolderLoader(items, 4, 16, device="cpu", **kw)):
        ld = make(batch_shard=(2, 3))                                            # two batches, three ranks
        assert len(ld) == 0 and ld.items == [] and tuple(ld.batch_range) == (2, 2) and list(ld) == []
        if hasattr(ld, "warm"):
            assert ld.warm() is ld
        cli._report_pipeline({}, "test set", ld)
        with pytest.raises(ValueError, match="ragged"):
            make(batch_shard=(0, 2), ragged=True, num_classes=1)
        with pytest.raises(ValueError, match="rank"):
            make(batch_shard=(2, 2))
    # independent of the class sharding: a class-sharded loader is not batch-sharded and the other way round
    assert cli.FolderLoader(items, 4, 16, 0, 2, 1).batch_shard is None and cli.FolderLoader(items, 4, 16, 0, 2, 1).presharded


# ----------------------------------------------------------------------------- 2. the evaluator under gloo
C, ROWS, BATCH = 5, 11, 4
EV_CONFIGS = [(topk, detail) for topk in (1, 2) for detail in (False, True)]


def _rows():
    """11 rows over 5 classes: row 2 ties its two largest columns, row 5 holds a NaN, row 9 carries a label outside [0, C)."""
    g = torch.Generator().manual_seed(3)
    mo = torch.rand((ROWS, C), generator=g)
    gt = torch.randint(0, C, (ROWS,), generator=g)
    mo[torch.arange(0, ROWS, 2), gt[::2]] += 1.0
    mo[2, 1] = mo[2, 3] = 2.0
    mo[5, 4] = float("nan")
    gt[9] = 7
    return mo, gt


def _state(ev):
    return {k: None if getattr(ev, k) is None else getattr(ev, k).clone() for k in ("_counts", "_hits", "_class_hits", "_cmat")}


def _evaluators(topk, detail, batches):
    """The TWO evaluators of one pass (the second sees the rows' columns reversed), having counted `batches`."""
    from ovmr_amd.evaluator import Classification
    mo, gt = _rows()
    evs = [Classification(C, device="cpu", per_class=detail, confusion=detail) for _ in range(2)]
    for ev in evs:
        ev.begin(topk)
    for b in batches:
        rows = slice(b * BATCH, min((b + 1) * BATCH, ROWS))
        evs[0].process(mo[rows], gt[rows], topk=topk)
        evs[1].process(mo[rows].flip(1), gt[rows], topk=topk)
    return evs


def _evaluator_rank(rank, world, port, out_dir):
    _open_group(rank, world, port)
    from ovmr_amd.evaluator import Classification
    from ovmr_amd.shard import shard_range
    calls = _count_all_reduces()
    first, end = shard_range(-(-ROWS // BATCH), rank, world)
    out = {"batches": (first, end)}
    for topk, detail in EV_CONFIGS:
        evs = _evaluators(topk, detail, range(first, end))
        before = len(calls)
        Classification.all_reduce(evs, dist)
        out[(topk, detail)] = {"states": [_state(ev) for ev in evs], "calls": calls[before:]}
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("world", [2, 3, 4])
def test_evaluator_state_summed_over_gloo_ranks(tmp_path, world):
    mp.spawn(_evaluator_rank, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    ranks = [torch.load(tmp_path / f"rank{r}.pt") for r in range(world)]
    assert [r["batches"] for r in ranks] == {2: [(0, 2), (2, 3)], 3: [(0, 1), (1, 2), (2, 3)], 4: [(0, 1), (1, 2), (2, 3), (3, 3)]}[world]
    for topk, detail in EV_CONFIGS:
        want = [_state(ev) for ev in _evaluators(topk, detail, range(3))]        # the one-process pass
        assert (want[0]["_hits"] is not None) == (topk > 1) and (want[0]["_cmat"] is not None) == detail
        assert (want[0]["_class_hits"] is not None) == (detail and topk > 1)
        assert int(want[0]["_counts"][3 * C]) == 1                                # the label outside [0, C) was counted as such
        small = 2 * (3 * C + 1 + (1 if topk > 1 else 0) + (C if detail and topk > 1 else 0))
        for r in ranks:
            got = r[(topk, detail)]
            for ev_got, ev_want in zip(got["states"], want):
                for k, t in ev_want.items():
                    assert (ev_got[k] is None) == (t is None), k
                    if t is not None:
                        assert ev_got[k].dtype == torch.int32 and torch.equal(ev_got[k], t), (world, topk, detail, k)
            # ONE all-reduce for the small counters of both evaluators, one per confusion matrix
            assert got["calls"] == [(small,)] + ([(C, C)] * 2 if detail else [])


def test_all_reduce_refuses_an_evaluator_that_has_not_begun():
    from ovmr_amd.evaluator import Classification
    ev = Classification(C, device="cpu")
    with pytest.raises(RuntimeError, match="begin"):
        Classification.all_reduce([ev], dist)
    ev.begin(2)
    assert ev._hits is not None and int(ev._hits) == 0 and ev._cmat is None
    with pytest.raises(ValueError, match="began already"):
        ev.begin(2)
    mo, gt = _rows()
    with pytest.raises(ValueError, match="one topk"):
        ev.process(mo, gt)                                                       # begin(2) fixed the pass's topk
    ev.process(mo, gt, topk=2)
    plain = Classification(C, device="cpu")
    plain.process(mo, gt, topk=2)                                                # without begin(): today's behaviour
    assert torch.equal(plain._counts, ev._counts) and torch.equal(plain._hits, ev._hits)


# ----------------------------------------------------------------------------- 3. _EvalTrainer.test() under gloo
T_ROWS, T_BATCH = 7, 4
TR_CONFIGS = [("fusion", 2, True), ("all", 2, True), ("all", 1, False)]           # (EVAL_MODE, TEST.TOPK, detail flags)


def _planes():
    g = torch.Generator().manual_seed(9)
    labels = torch.tensor([0, 0, 1, 2, 2, 3, 4])
    planes = []
    for share in (0.9, 0.4, 0.7, 0.2):
        x = torch.rand((T_ROWS, C), generator=g)
        hit = torch.rand(T_ROWS, generator=g) < share
        x[torch.arange(T_ROWS)[hit], labels[hit]] += 2.0
        planes.append(torch.softmax(4 * x, 1))
    return torch.stack(planes), labels


class _Batches(list):
    batch_shard = None


def _loader(batch_shard):
    from ovmr_amd.shard import keep_batch_shard
    _, labels = _planes()
    mine, shard, _ = keep_batch_shard(list(range(T_ROWS)), T_BATCH, batch_shard)
    out = _Batches({"img": torch.tensor(mine[s:s + T_BATCH]), "label": labels[mine[s:s + T_BATCH]]} for s in range(0, len(mine), T_BATCH))
    out.batch_shard = shard
    return out


def _trainer(mode, topk, detail, out_dir, loader):
    from ovmr_amd import modules, trainer
    stacked, _ = _planes()

    class StandIn(trainer._EvalTrainer):
        def build_model(self):
            pass

        def outputs(self, inputs):
            for x in inputs:                                 # an "image" batch is its rows' indices
                yield stacked[:, x] if mode == "all" else stacked[0][x]

    cfg = modules.make_cfg(output_dir=out_dir, eval_mode=mode)
    cfg.TEST = SimpleNamespace(SPLIT="test", TOPK=topk)
    dm = SimpleNamespace(dataset=SimpleNamespace(classnames=[f"class {c}" for c in range(C)]), test_loader=loader, val_loader=None)
    flags = dict(per_class_result=True, compute_cmat=True) if detail else {}
    return StandIn(cfg, dm, device="cpu", **flags)


def _files(d):
    out = {}
    for root, _, names in os.walk(d):
        for n in names:
            with open(os.path.join(root, n), "rb") as f:
                out[os.path.relpath(os.path.join(root, n), d)] = f.read()
    return out


def _pass(mode, topk, detail, out_dir, loader):
    t = _trainer(mode, topk, detail, out_dir, loader)
    buf = io.StringIO()
    with redirect_stdout(buf):
        first = t.test()
    return {"results": dict(t.results), "first": first, "text": buf.getvalue().replace(out_dir, "DIR"), "files": _files(out_dir)}


def _trainer_rank(rank, world, port, tmp):
    _open_group(rank, world, port)
    calls = _count_all_reduces()
    out = {}
    # a loader of another world than the group's is refused before the first batch (no collective is entered)
    try:
        _trainer("fusion", 1, False, "", _loader((rank, world + 1))).test()
        out["refused"] = ""
    except RuntimeError as e:
        out["refused"] = str(e)
    assert not calls
    for i, (mode, topk, detail) in enumerate(TR_CONFIGS):
        before = len(calls)
        out[i] = _pass(mode, topk, detail, os.path.join(tmp, f"cfg{i}_rank{rank}"), _loader((rank, world)))
        out[i]["calls"] = calls[before:]
    # an unsharded loader under a process group: every rank evaluates everything, nothing is reduced
    before = len(calls)
    out["unsharded"] = _pass("all", 2, True, os.path.join(tmp, f"unsharded_rank{rank}"), _loader(None))
    out["unsharded"]["calls"] = calls[before:]
    torch.save(out, os.path.join(tmp, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("world", [2, 3])
def test_trainer_pass_over_gloo_ranks_equals_one_process(tmp_path, world):
    mp.spawn(_trainer_rank, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    ranks = [torch.load(tmp_path / f"rank{r}.pt") for r in range(world)]
    assert all("batch_shard" in r["refused"] and f"of {world + 1}" in r["refused"] for r in ranks)
    for i, (mode, topk, detail) in enumerate(TR_CONFIGS):
        one = _pass(mode, topk, detail, str(tmp_path / f"one{i}"), _loader(None))
        n_ev = 4 if mode == "all" else 1
        assert len(one["files"]) == n_ev * (3 if detail else 2) and "=> result\n" in one["text"]
        small = n_ev * (3 * C + 1 + (1 if topk > 1 else 0) + (C if detail and topk > 1 else 0))
        for rank, r in enumerate(ranks):
            got = r[i]
            assert got["results"] == one["results"] and list(got["results"]) == list(one["results"]) and got["first"] == one["first"]
            assert got["calls"] == [(small,)] + ([(C, C)] * n_ev if detail else []), (world, rank, i)
            if rank == 0:
                assert got["text"] == one["text"] and got["files"] == one["files"]
            else:                                            # ranks > 0 wrote nothing and printed no result block
                assert got["files"] == {} and not os.path.exists(tmp_path / f"cfg{i}_rank{rank}")
                assert got["text"] == "Evaluate on the *test* set\n"
    one = _pass("all", 2, True, str(tmp_path / "one_unsharded"), _loader(None))
    for r in ranks:
        got = r["unsharded"]
        assert got["calls"] == [] and got["results"] == one["results"] and got["text"] == one["text"] and got["files"] == one["files"]


def test_sharded_loader_without_a_process_group_raises():
    assert not dist.is_initialized()
    seen = []
    t = _trainer("fusion", 1, False, "", _loader((0, 2)))
    t.outputs = lambda inputs: seen.append(1) or iter(())
    with pytest.raises(RuntimeError, match="no torch.distributed process group"):
        t.test()
    assert not seen and not hasattr(t, "results")                                # refused before the first batch
    _trainer("fusion", 1, False, "", _loader((0, 1))).test()                      # a world of one is the one-process pass
