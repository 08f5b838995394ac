"""Runner for the generation / evaluation modes of the reference's train.py.

    python -m ovmr_amd.cli --eval-only --trainer MM_CLS_OP \\
        --root DATA --clip-weights ViT-B-16.pt --bpe-path bpe_simple_vocab_16e6.txt.gz \\
        --model-dir ./checkpoints --load-epoch 30 --output-dir output_ovmr/generated_classifiers \\
        --eval_mode fusion --eval_tau 10 --n_ctx 2  DATASET.NUM_SHOTS 16

    python -m ovmr_amd.cli --eval-only --trainer ZeroshotCLIP2 --root DATA --clip-weights ViT-B-16.pt \\
        --bpe-path bpe_simple_vocab_16e6.txt.gz --output-dir output/zsclip2 DATASET.NAME Caltech101

runs the zero-shot trainers of trainers/zsclip.py on the same folder data set, and

    python -m ovmr_amd.cli --eval-only --trainer MM_CLS_OP ... --predict IMAGES --topk 5 [--classifiers OUTPUT_DIR/mm_classifiers.pt]

ranks the job's classes for UNLABELLED images (a directory, or a text file of paths) instead of the test pass: OUTPUT_DIR/predictions.csv holds
`image,rank,label,classname,score` (any of the three trainers; `--classifiers` loads a generated file instead of generating again).
With `--nearest N` (MM_CLS_OP, after a generation in this run or from `--bank`; 1 <= N <= 32) OUTPUT_DIR/neighbours.csv also holds
`image,rank,label,classname,neighbour,row,exemplar,similarity`: the N nearest exemplars of every (image, predicted class), predictions.csv unchanged.

    python -m ovmr_amd.cli --eval-only --trainer MM_CLS_OP ... --bank OUT/reference_bank.pt --audit-bank 5 [--dup-threshold T]

audits the exemplar features themselves: OUTPUT_DIR/bank_audit.csv (one line per exemplar: its nearest class-mate, its nearest image of
another class, `suspect` where the latter is strictly closer, `duplicate_of`), bank_audit_neighbours.csv and bank_audit_classes.csv.  From
`--bank` alone nothing is decoded or encoded and no `--root` is needed; it also runs after a generation or an edit, and next to `--predict`.

    python -m ovmr_amd.cli --eval-only --trainer MM_CLS_OP ... --retrieve IMAGES [--per-class M] [--within-top K]

searches an UNLABELLED image pool (listed as `--predict` lists it) by class instead of the test pass: OUTPUT_DIR/retrieval.csv holds
`label,classname,rank,image,score`, the M (default 32, at most 32) best images of every class in class order then rank, equal scores to the
image listed first; with `--within-top K` a class is searched only among the images that rank it within their K best scores (ties at the
cut included).  Any of the three trainers; after a generation, from `--classifiers FILE`, or from `--bank FILE` without `--root`.  Not with
`--predict`, `--eval_mode all` or the test pass's detail flags.  Under `torch.distributed.run` the pool's batches are sharded over the
ranks like the test pass's, the per-class lists are all-gathered and merged on every rank, and rank 0 writes the one-process file byte for
byte (`--predict` stays one process).

    python -m ovmr_amd.cli --eval-only --trainer MM_CLS_OP ... --eval_mode all

evaluates the four modes of the reference's result tables (fusion, text, vision, multimodal; trainers/mm_classifier_one_prompt.py:348-363)
in ONE test pass -- the exemplars are drawn, the classifiers generated and every test image decoded and encoded once instead of four
times: a `=> eval mode: <mode>` line and the result block per mode, a four-line summary, the results keyed `<mode>/accuracy` ..., and
acc_per_class.csv / f1_per_class.csv / cmat.pt in OUTPUT_DIR/<mode>/ (mm_classifiers.pt / visual_tokens.pt in OUTPUT_DIR, once).  Each
mode's figures and files are those of its own single-mode run.  Not with `--predict` (a ranked prediction needs one mode); the zero-shot
trainers ignore EVAL_MODE.

    python -m ovmr_amd.cli --eval-only --trainer ZeroshotCLIP ... --per-class-result --confusion-matrix

adds the reference's `=> per-class result` block (and `perclass_accuracy` in the results) and OUTPUT_DIR/cmat.pt, the row-normalised
confusion matrix, to the test pass of any of the three trainers.  These two FLAGS are the switch: the reference's keys
`TEST.PER_CLASS_RESULT` / `TEST.COMPUTE_CMAT` stay accepted and ignored.  They do not go with `--predict`.  Either way `main` is train.py's evaluation path,
`trainer.build_trainer(cfg, dm, ...)` and `.test()` (ovmr_amd/trainer.py), on loaders of this runner's own.  Under
`python -m torch.distributed.run --nproc-per-node N -m ovmr_amd.cli ...` (any of the three trainers; not `--predict`) the runner opens the process
group, shards the classes over the ranks for the generation and the BATCHES of the test set for the test pass: every rank evaluates its own
contiguous range of the one-process pass's batches, the evaluator's counters are summed over the ranks, rank 0 prints and writes -- the figures and
files of the one-process job byte for byte -- and every rank returns the results plus `test_shard` (its rank, world, batch range, images).  It
takes the command line of `scripts/mm_cls/generate_classifier.sh:30-44` / `train.py:183-255` as it is: `--dataset-config-file` and
`--config-file` (YAML, read with PyYAML), the flags `reset_cfg` copies (`--root --output-dir --seed --trainer --backbone --init_weight
--n_ctx --eval_mode --eval_tau`) and the trailing `KEY VALUE` opts, merged in train.py's order by `ovmr_amd.config.setup_cfg` with the
reference's defaults (EVAL_MODE multimodal, N_CTX 16, DATALOADER.TEST.BATCH_SIZE 32, bilinear resize and NO normalisation unless the
config file says otherwise -- exactly what train.py does without its YAML files).  Keys this path honours: `DATASET.NUM_SHOTS`,
`DATASET.SUBSAMPLE_CLASSES` (all | base | new, datasets/oxford_pets.py:141-202), `DATALOADER.TEST.BATCH_SIZE`, `DATALOADER.NUM_WORKERS`,
`INPUT.SIZE / INTERPOLATION / PIXEL_MEAN / PIXEL_STD / TRANSFORMS`, `TRAINER.COCOOP.N_CTX`, `MODEL.BACKBONE.NAME`, `MODEL.INIT_WEIGHTS`,
`EVAL_MODE`, `EVAL_TAU`, `SEED`, `OUTPUT_DIR`, `TEST.TOPK`; training / optimiser keys are accepted and ignored; any other key raises.  yacs / Dassl
are not needed; `--transforms` sets INPUT.TRANSFORMS as in train.py:69-70, train.py's remaining flags (`--source-domains --target-domains
--fs_classifier --head --stage_num --visual_token_path`) are accepted and ignored.  Extra flags of this runner: `--clip-weights` (no download here), `--bpe-path`, `--eval-split / --test-split`, the
input-pipeline knobs, `--exemplar-list`.  Data layout (datasets/imagenet.py:146-159):
`<root>/<split>/<class folder>/<image>`; `<root>/classnames.txt` lines "<folder> <class name>" (optional: folder names
are used otherwise).  The exemplar (eval) set is NUM_SHOTS images per class folder of `--eval-split` (default "train") drawn
under `--seed` exactly as the reference's generate_fewshot_dataset draws them, the test set is every image of `--test-split`
(default "val").

Vocabulary edits (MM_CLS_OP only; DESIGN.md section 6, ovmr_amd/bank.py):

    python -m ovmr_amd.cli --eval-only --trainer MM_CLS_OP ... --save-bank
    python -m ovmr_amd.cli --eval-only --trainer MM_CLS_OP ... --bank OLD/reference_bank.pt --output-dir NEW \\
        [--remove-classes NAME [NAME ...]] [--replace-classes DIR] [--add-classes DIR] [--predict IMAGES | the test pass]

`--save-bank` makes a generation job also write OUTPUT_DIR/reference_bank.pt (vocabulary, exemplar features and their paths, classifiers,
tokens, counters, fusion weights).  `--bank FILE` starts from such a file instead of generating: no exemplar is decoded; with `--predict`
neither `--root` nor a data-set folder is needed (the class names come from the bank), with a test pass the data set's class names must
equal the bank's (after the edits), in order.  `--add-classes DIR` / `--replace-classes DIR`: one sub-folder of images per class (sorted
folder order = append order; names from DIR/classnames.txt, else the folder name; a replaced folder must name an existing class), its
exemplars drawn under `--seed` and DATASET.NUM_SHOTS as for a data set (`--ragged-shots`: the ragged layout).  `--remove-classes` takes
class names (put another flag, not the KEY VALUE opts, behind the list).  The edits apply in the order remove, replace, add; only the
named classes are decoded and generated.  The edited model writes mm_classifiers.pt, visual_tokens.pt and reference_bank.pt into
OUTPUT_DIR and goes on to the test pass or `--predict`.  One process only.

Input pipeline (ovmr_amd/loader.py): `--workers` processes DECODE into a page-locked shared ring, a side stream uploads a batch and runs
ovmr_resize_crop_u8 (Resize + CenterCrop, bit-equal to PIL) and ovmr_preprocess_u8 (normalise + fp16) on the GPU while the encoder
works on the previous one; `--host-resize` keeps the resize in the workers.  JPEG decode on the host's cores remains the bound of the
whole job (profiles/r05e_pipeline_bench_device_vs_host_resize.log: 14.5 k images/s with 16 workers against ~30 k for the encoder): the
runner prints end-to-end images/s and the share of the time the host waited for the decoders.
"""
from __future__ import annotations

import argparse
import os
import os.path as osp
import sys
from types import SimpleNamespace
from typing import Dict, List, Sequence, Tuple

import numpy as np            # (torch is imported inside the functions: under `python -m ovmr_amd.cli` the spawned decode workers
                              #  re-import this module as __mp_main__ and must stay torch-free)

PIXEL_MEAN = (0.48145466, 0.4578275, 0.40821073)      # configs/trainers/MM_CLS_OP/*.yaml:14-15
PIXEL_STD = (0.26862954, 0.26130258, 0.27577711)


def test_transform(img, size: int = 224, interpolation: str = "bicubic", mean=PIXEL_MEAN, std=PIXEL_STD) -> torch.Tensor:
    """_build_transform_test (Dassl.pytorch/dassl/data/transforms/transforms.py:495-526): resize of the smaller edge to `size`
    (INPUT.INTERPOLATION; the MM_CLS_OP configs say bicubic), center crop, [0,1] tensor, normalise with INPUT.PIXEL_MEAN / PIXEL_STD
    (`mean=None`: no Normalize, what the reference does when "normalize" is not in INPUT.TRANSFORMS, :514-518)."""
    import torch
    from ._decode_worker import load_u8
    x = torch.from_numpy(load_u8(img, size, interpolation=interpolation).copy()).permute(2, 0, 1).float().div_(255.0)
    if mean is None:
        return x
    return (x - torch.tensor(tuple(mean)).view(3, 1, 1)) / torch.tensor(tuple(std)).view(3, 1, 1)


def list_split(root: str, split: str) -> Tuple[List[str], List[Tuple[str, int]]]:
    """datasets/imagenet.py:146-159: sorted class folders -> labels 0..C-1, every non-hidden file is an image."""
    d = osp.join(root, split)
    folders = sorted(f.name for f in os.scandir(d) if f.is_dir())
    items = []
    for label, folder in enumerate(folders):
        for name in sorted(n for n in os.listdir(osp.join(d, folder)) if not n.startswith(".")):
            items.append((osp.join(d, folder, name), label))
    return folders, items


def read_classnames(root: str, folders: Sequence[str]) -> List[str]:
    path = osp.join(root, "classnames.txt")
    names: Dict[str, str] = {}
    if osp.exists(path):
        with open(path) as f:
            for line in f:
                parts = line.strip().split(" ")
                if parts and parts[0]:
                    names[parts[0]] = " ".join(parts[1:])
    return [names.get(f, f) for f in folders]


class FolderLoader:
    """Iterable of {"img", "label"} dict batches (the loader protocol of SURVEY.md 8b).

    With world > 1 the loader is class-sharded: a rank keeps only the items whose class lies in its contiguous
    `shard_range` of the `num_classes` classes, so it opens and decodes only its own images; `presharded = True` then tells
    CustomCLIP.forward_prompt that every batch it receives is its own.

    batch_shard=(rank, world) shards a TEST pass instead, independently of the above: the loader keeps the items of its contiguous range
    of the one-process loader's batches (shard.shard_test_batches: same item order, same batch boundaries) and publishes `.batch_shard`
    and `.batch_range` = [first, end) of those batches; `_EvalTrainer.test()` then sums the evaluator state over the ranks.  A rank whose
    range is empty has a loader of zero batches."""

    def __init__(self, items: Sequence[Tuple[str, int]], batch_size: int, size: int, rank: int = 0, world: int = 1,
                 num_classes: int = 0, interpolation: str = "bicubic", mean=PIXEL_MEAN, std=PIXEL_STD, ragged: bool = False,
                 batch_shard=None):
        """ragged: `items` is a ragged exemplar set (layout_exemplars_ragged).  A batch then holds whole classes, at most
        `batch_size` rows, and carries "shots" (host int64 [n_cls]); `.shots` is int32 [C], the rows of every class of the vocabulary."""
        self.bs, self.size = batch_size, size
        self.tfm = dict(interpolation=interpolation, mean=mean, std=std)
        self.presharded = world > 1
        from .shard import keep_batch_shard, ragged_batches, shard_range, vocabulary_shots
        self.shots = vocabulary_shots(items, num_classes) if ragged else None
        if world > 1:
            lo, hi = shard_range(num_classes or (1 + max(l for _, l in items)), rank, world)
            items = [it for it in items if lo <= it[1] < hi]
        self.items, self.batch_shard, self.batch_range = keep_batch_shard(list(items), int(batch_size), batch_shard, ragged)
        if ragged:
            self.spans = ragged_batches(self.items, self.bs)
        else:
            self.spans = [(s, min(s + self.bs, len(self.items)), None) for s in range(0, len(self.items), self.bs)]

    def __len__(self):
        return len(self.spans)

    def __iter__(self):
        import torch
        for a, b, shots in self.spans:
            chunk = self.items[a:b]
            imgs = torch.stack([test_transform(p, self.size, **self.tfm) for p, _ in chunk])
            batch = {"img": imgs, "label": torch.tensor([l for _, l in chunk], dtype=torch.long)}
            if shots is not None:
                batch["shots"] = torch.tensor(shots, dtype=torch.long)
            yield batch


def fewshot_items(items: Sequence[Tuple[str, int]], shots: int, seed: int = 1) -> List[Tuple[str, int]]:
    """The few-shot subset, drawn as the reference draws it: `random.seed(SEED)` (set_random_seed, train.py:183-186), then per
    class, in order of first appearance, `random.sample(items_of_the_class, NUM_SHOTS)`; a class with fewer images keeps them
    all and draws nothing (Dassl.pytorch/dassl/data/datasets/base_dataset.py:175-205 generate_fewshot_dataset, repeat=False).
    The sampling PROCEDURE is the reference's (tests/golden/fewshot.npz holds the reference's picks for the same item lists); the
    same images as a reference run additionally need the same item ORDER inside a class: the reference lists a class folder in
    raw os.listdir order (listdir_nohidden(sort=False), datasets/imagenet.py:149), this runner sorts the names.  To reproduce a
    particular reference run, hand its exemplar set over with `--exemplar-list`.  seed < 0: unseeded, as train.py:157-159."""
    import random
    rng = random.Random(seed) if seed >= 0 else random.Random()    # the stream of the global generator after random.seed(seed)
    per: Dict[int, List[Tuple[str, int]]] = {}
    for it in items:
        per.setdefault(it[1], []).append(it)
    out = []
    for its in per.values():
        out.extend(rng.sample(its, shots) if len(its) >= shots else its)
    return out


def exemplar_items(items: Sequence[Tuple[str, int]], shots: int, seed: int = 1) -> List[Tuple[str, int]]:
    """`fewshot_items` laid out for the eval-set loader: exactly NUM_SHOTS consecutive rows per class.  A class
    with fewer images is filled up with replacement, as RandomClassSampler does (samplers.py:148-149, there from numpy's global
    generator at iteration time; here from RandomState(seed)).  The reference additionally shuffles the order of the shots and
    of the classes (samplers.py:117-181), which the path does not depend on: the aggregator has no positional embedding."""
    return layout_exemplars(fewshot_items(items, shots, seed), shots, seed)


def layout_exemplars(few: Sequence[Tuple[str, int]], shots: int, seed: int = 1) -> List[Tuple[str, int]]:
    """The eval-set loader's row order for an already drawn few-shot subset (see `exemplar_items`)."""
    per: Dict[int, List[Tuple[str, int]]] = {}
    for it in few:
        per.setdefault(it[1], []).append(it)
    fill = np.random.RandomState(seed if seed >= 0 else None)
    out = []
    for label, its in per.items():
        if len(its) > shots:
            # forward_prompt groups rows purely by position (num_cls = B // S, label.reshape(num_cls, S)[:, 0],
            # trainers/mm_classifier_one_prompt.py:237-240): one surplus row would shift every later class group.  The reference's
            # RandomClassSampler emits exactly n_ins rows per class (samplers.py:117-181); a list with more is refused, not trimmed
            raise ValueError(f"class {label} has {len(its)} exemplar rows, more than DATASET.NUM_SHOTS = {shots}")
        if len(its) < shots:
            its = its + [its[int(k)] for k in fill.choice(len(its), size=shots - len(its), replace=True)]
        out.extend(its)
    return out


def layout_exemplars_ragged(few: Sequence[Tuple[str, int]], shots: int) -> List[Tuple[str, int]]:
    """The eval-set loader's row order in ragged mode (`--ragged-shots`): every class's rows consecutively, classes in order of first
    appearance, a class's rows in the order given -- and exactly the rows given: a class with fewer than NUM_SHOTS images is NOT filled
    up (a duplicate would double an exemplar's weight in the aggregator's softmax and vote twice in the F1 preference).  More than
    NUM_SHOTS rows are refused as in `layout_exemplars`, a row listed twice as well."""
    per: Dict[int, List[Tuple[str, int]]] = {}
    for it in few:
        per.setdefault(it[1], []).append(it)
    out = []
    for label, its in per.items():
        if len(its) > shots:
            raise ValueError(f"class {label} has {len(its)} exemplar rows, more than DATASET.NUM_SHOTS = {shots}")
        if len({p for p, _ in its}) != len(its):
            raise ValueError(f"class {label} lists an exemplar image twice: a ragged exemplar set holds no duplicates")
        out.extend(its)
    return out


def read_exemplar_list(path: str, num_classes: int, shots: int) -> List[Tuple[str, int]]:
    """`--exemplar-list`: one `<image path> <label>` per line.  Checked before anything is decoded: every label inside
    [0, num_classes), every file present, at most NUM_SHOTS rows per class (fewer are filled up with replacement by
    `layout_exemplars`, as RandomClassSampler does; under `--ragged-shots` they stay as they are) -- a malformed list fails here with the offending line, not as shifted class
    groups inside forward_prompt."""
    few: List[Tuple[str, int]] = []
    per: Dict[int, int] = {}
    with open(path) as f:
        for no, raw in enumerate(f, 1):
            ln = raw.strip()
            if not ln:
                continue
            parts = ln.rsplit(" ", 1)
            if len(parts) != 2 or not parts[1].lstrip("-").isdigit():
                raise SystemExit(f"{path}:{no}: expected `<image path> <label>`, got {ln!r}")
            img, label = parts[0], int(parts[1])
            if not 0 <= label < num_classes:
                raise SystemExit(f"{path}:{no}: label {label} outside [0, {num_classes}) -- the labels are the class-folder indices BEFORE class subsampling")
            if not os.path.isfile(img):
                raise SystemExit(f"{path}:{no}: image {img!r} does not exist")
            per[label] = per.get(label, 0) + 1
            if per[label] > shots:
                raise SystemExit(f"{path}:{no}: class {label} has more than DATASET.NUM_SHOTS = {shots} exemplars (the eval-set loader "
                                 "carries exactly NUM_SHOTS rows per class; trim the list or raise NUM_SHOTS)")
            few.append((img, label))
    if not few:
        raise SystemExit(f"{path}: no exemplars listed")
    return few


IMAGE_EXTENSIONS = (".jpg", ".jpeg", ".png", ".bmp", ".gif", ".ppm", ".pgm", ".tif", ".tiff", ".webp")
PREDICT_ONE_PROCESS = "--predict runs in one process: sharding the prediction pass over ranks is not implemented"
MAX_TOPK = 32                 # ovmr_topk_rows (include/ovmr_hip.h)


def list_predict_images(path: str, flag: str = "--predict") -> List[str]:
    """`--predict PATH` (and `--retrieve PATH`: `flag` names the one in the messages): a directory -- every image file below it (IMAGE_EXTENSIONS, hidden names skipped), sorted by path -- or a text
    file with one image path per line, in file order.  Checked before anything is loaded: an empty PATH or a missing file is a SystemExit
    that names it."""
    if not path:
        raise SystemExit(f"{flag}: PATH is empty (a directory of images, or a text file with one image path per line)")
    if osp.isdir(path):
        images = []
        for d, dirs, files in os.walk(path):
            dirs[:] = [x for x in dirs if not x.startswith(".")]
            images += [osp.join(d, n) for n in files if not n.startswith(".") and n.lower().endswith(IMAGE_EXTENSIONS)]
        if not images:
            raise SystemExit(f"{flag} {path!r}: no image file below this directory ({', '.join(IMAGE_EXTENSIONS)})")
        return sorted(images)
    if not osp.isfile(path):
        raise SystemExit(f"{flag} {path!r}: no such directory or list file")
    images = []
    with open(path) as f:
        for no, raw in enumerate(f, 1):
            img = raw.strip()
            if not img:
                continue
            if not osp.isfile(img):
                raise SystemExit(f"{path}:{no}: image {img!r} does not exist")
            images.append(img)
    if not images:
        raise SystemExit(f"{flag} {path!r}: the list names no image")
    return images


def ranked_predictions(paths: Sequence[str], values, indices, classnames: Sequence[str]):
    """[(path, [(label, classname, score), ...k])] from the [N, k] values / indices of a prediction pass."""
    return [(p, [(int(c), classnames[int(c)], float(v)) for v, c in zip(vs, cs)]) for p, vs, cs in zip(paths, values.tolist(), indices.tolist())]


def _write_csv(path: str, columns: Sequence[str], lines, float_columns=()) -> None:
    """The writer behind every table of the runner: the header, then one line per entry of `lines` in order; the columns whose
    positions float_columns names are written as repr(float), so they parse back to the same value.  Creates the directory."""
    import csv
    os.makedirs(osp.dirname(path) or ".", exist_ok=True)
    with open(path, "w", newline="") as f:
        w = csv.writer(f, delimiter=",", lineterminator="\n")
        w.writerow(columns)
        for line in lines:
            w.writerow([repr(float(x)) if i in float_columns else x for i, x in enumerate(line)])


def write_predictions(path: str, predictions) -> None:
    """predictions.csv: `image,rank,label,classname,score`, one line per (image, rank) in input order, ranks 0..k-1; the score is
    repr(float), so it parses back to the same value."""
    lines = [(image, rank, label, name, score) for image, ranks in predictions for rank, (label, name, score) in enumerate(ranks)]
    _write_csv(path, ["image", "rank", "label", "classname", "score"], lines, (4,))


MAX_PER_CLASS = 32            # ovmr_retrieve_update (include/ovmr_hip_retrieve.h)
MAX_POOL = 2 ** 32 - 1        # image indices of a pool lie in [0, 2^32 - 1)
RETRIEVAL_COLUMNS = ["label", "classname", "rank", "image", "score"]


def check_retrieve(args, trainer_name: str, zeroshot: bool, eval_mode: str):
    """The refusals of `--retrieve PATH [--per-class M] [--within-top K]`, before anything is listed or loaded."""
    if args.retrieve is None:
        for flag, v in (("--per-class M", args.per_class), ("--within-top K", args.within_top)):
            if v is not None:
                raise SystemExit(f"{flag} belongs to --retrieve PATH: the search of an image pool by class")
        return
    if args.predict is not None:
        raise SystemExit("--retrieve searches a pool by class, --predict ranks the classes of every image: one of the two per run")
    if eval_mode == "all" and not zeroshot:
        raise SystemExit("--retrieve searches under ONE mode: --eval_mode all belongs to the test pass (fusion, text, vision or multimodal here)")
    for flag, on in (("--per-class-result", args.per_class_result), ("--confusion-matrix", args.confusion_matrix)):
        if on:
            raise SystemExit(f"{flag} belongs to the test pass: --retrieve searches unlabelled images, there is nothing to count")
    if args.topk is not None:
        raise SystemExit("--topk K belongs to --predict PATH (--retrieve takes --per-class M and --within-top K)")
    m = MAX_PER_CLASS if args.per_class is None else args.per_class
    if not 1 <= m <= MAX_PER_CLASS:
        raise SystemExit(f"--per-class {m}: M must lie in [1, {MAX_PER_CLASS}]")
    if args.within_top is not None and not 1 <= args.within_top <= MAX_TOPK:
        raise SystemExit(f"--within-top {args.within_top}: K must lie in [1, min({MAX_TOPK}, number of classes)]")


MAX_BINS = 4096               # ovmr_eval_curves (include/ovmr_hip_curves.h)
DEFAULT_BINS = 256


def check_score_curves(args, trainer_name: str, zeroshot: bool):
    """The refusals of `--score-curves [BINS] [--score-range LO HI]`, before anything is listed or loaded -> (bins, (lo, hi)), or
    (None, None) without the flag.  MM_CLS_OP's outputs are probabilities: the range defaults to 0 1.  The zero-shot trainers return
    logits, which have no natural range: there the range must be given."""
    import math
    if args.score_curves is None:
        if args.score_range is not None:
            raise SystemExit("--score-range LO HI belongs to --score-curves [BINS]: the range the score histograms of the test pass cover")
        return None, None
    for flag, v in (("--predict", args.predict), ("--retrieve", args.retrieve)):
        if v is not None:
            raise SystemExit(f"--score-curves belongs to the test pass: {flag} reads unlabelled images, a score has no label to be held against")
    bins = args.score_curves
    if not 1 <= bins <= MAX_BINS:
        raise SystemExit(f"--score-curves {bins}: BINS must lie in [1, {MAX_BINS}]")
    if args.score_range is None:
        if zeroshot:
            raise SystemExit(f"--score-curves: --trainer {trainer_name} returns logits, which have no natural range: give --score-range LO HI")
        return bins, (0.0, 1.0)
    lo, hi = args.score_range
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise SystemExit(f"--score-range {lo} {hi}: LO and HI must be finite")
    if not lo < hi:
        raise SystemExit(f"--score-range {lo} {hi}: LO must lie below HI")
    from .runtime import curve_scale
    try:
        curve_scale(lo, hi, bins, "--score-range")
    except ValueError:
        raise SystemExit(f"--score-range {lo} {hi}: as fp32 the range must be finite, increasing and wide enough for {bins} bins") from None
    return bins, (lo, hi)


DEFAULT_EXACT_GIB = 16.0


def check_exact_curves(args):
    """The refusals of `--exact-curves [--exact-budget GIB]`, before anything is listed or loaded -> (on, bytes of the score store's
    budget or None).  Any trainer will do: the exact figures take the scores as they are and need no range."""
    import math
    if not args.exact_curves:
        if args.exact_budget is not None:
            raise SystemExit("--exact-budget GIB belongs to --exact-curves: the memory the kept scores of the test pass may take")
        return False, None
    for flag, v in (("--predict", args.predict), ("--retrieve", args.retrieve)):
        if v is not None:
            raise SystemExit(f"--exact-curves belongs to the test pass: {flag} reads unlabelled images, a score has no label to be held against")
    gib = DEFAULT_EXACT_GIB if args.exact_budget is None else args.exact_budget
    if not (math.isfinite(gib) and gib > 0):
        raise SystemExit(f"--exact-budget {gib}: GIB must be a positive number of GiB")
    return True, int(gib * (1 << 30))


def check_pool_size(n: int, path: str):
    """An image's position in the pool takes the 32 low bits of a key, 2^32 - 1 excluded (include/ovmr_hip_retrieve.h)."""
    if n >= MAX_POOL:
        raise SystemExit(f"--retrieve {path!r}: a pool of {n:,} images; one search takes fewer than 2^32 - 1 = {MAX_POOL:,}")


def retrieval_rows(values, indices, images: Sequence[str], classnames: Sequence[str]):
    """[(label, classname, rank, image, score)] from the [C, m] values / indices of a search, class after class, best first; an unfilled
    rank (index -1) has no entry."""
    out = []
    for c, (vs, ix) in enumerate(zip(values.tolist(), indices.tolist())):
        out += [(c, classnames[c], rank, images[i], float(v)) for rank, (v, i) in enumerate(zip(vs, ix)) if i >= 0]
    return out


def write_retrieval(path: str, rows) -> None:
    """retrieval.csv: `label,classname,rank,image,score`, one line per filled (class, rank) in class order then rank; the score is
    repr(float), as in predictions.csv."""
    _write_csv(path, RETRIEVAL_COLUMNS, rows, (4,))


MAX_NEAREST = 32              # ovmr_nearest_rows (include/ovmr_hip_nearest.h)
NEIGHBOUR_COLUMNS = ["image", "rank", "label", "classname", "neighbour", "row", "exemplar", "similarity"]


def nearest_neighbours(paths: Sequence[str], indices, similarities, rows, classnames: Sequence[str], exemplar_paths=None):
    """[(image, class rank, label, classname, neighbour rank, bank row, exemplar path, similarity)] from the [N, k] indices and the
    [N, k, n] similarities / rows of a prediction pass with --nearest; a class with fewer than n exemplars (row -1) has fewer entries."""
    out = []
    for p, cs, ss, rs in zip(paths, indices.tolist(), similarities.tolist(), rows.tolist()):
        for rank, (c, sv, rv) in enumerate(zip(cs, ss, rs)):
            for j, (sim, row) in enumerate(zip(sv, rv)):
                if row >= 0:
                    out.append((p, rank, int(c), classnames[int(c)], j, int(row), "" if exemplar_paths is None else exemplar_paths[int(row)], float(sim)))
    return out


def write_neighbours(path: str, neighbours) -> None:
    """neighbours.csv: `image,rank,label,classname,neighbour,row,exemplar,similarity`, one line per (image, class rank, neighbour rank) in
    input order; the similarity is repr(float), as the score of predictions.csv."""
    _write_csv(path, NEIGHBOUR_COLUMNS, neighbours, (7,))


def check_nearest(args, trainer_name: str, zeroshot: bool):
    """The refusals of `--nearest N`, before anything is listed or loaded."""
    if args.nearest is None:
        return
    if args.predict is None:
        raise SystemExit("--nearest N belongs to --predict PATH: the nearest exemplars of every predicted class")
    if zeroshot:
        raise SystemExit(f"--nearest: --trainer {trainer_name} has no exemplars to search (MM_CLS_OP only; a zero-shot trainer's classifier rows are text features)")
    if args.classifiers:
        raise SystemExit(f"--nearest: --classifiers {args.classifiers!r} holds no exemplar features (generate in this run, or start from --bank)")
    if not 1 <= args.nearest <= MAX_NEAREST:
        raise SystemExit(f"--nearest {args.nearest}: N must lie in [1, {MAX_NEAREST}]")


AUDIT_COLUMNS = ["row", "label", "classname", "exemplar", "in_row", "in_similarity", "out_row", "out_label", "out_classname", "out_similarity",
                 "suspect", "duplicate_of"]
AUDIT_NEIGHBOUR_COLUMNS = ["row", "side", "rank", "neighbour_row", "neighbour_label", "similarity"]
AUDIT_CLASS_COLUMNS = ["label", "classname", "exemplars", "suspects", "duplicates"]
AUDIT_FILES = ("bank_audit.csv", "bank_audit_neighbours.csv", "bank_audit_classes.csv")


def bank_audit_tables(audit: dict, classnames: Sequence[str], shots: Sequence[int], exemplar_paths=None):
    """The three tables of `--audit-bank` from CustomCLIP.audit_bank's tensors (host or device): one line per exemplar (its first
    neighbour on either side; a missing one is row -1, label -1, an empty class name, similarity -inf), one per (exemplar, side, rank)
    for the neighbours that exist, one per class."""
    a = {k: v.cpu().tolist() for k, v in audit.items()}
    rows, neighbours = [], []
    for i, (row, label) in enumerate(zip(a["rows"], a["labels"])):
        ir, isim, orow, olab, osim = a["in_row"][i], a["in_sim"][i], a["out_row"][i], a["out_label"][i], a["out_sim"][i]
        rows.append((row, label, classnames[label], "" if exemplar_paths is None else exemplar_paths[row], ir[0], float(isim[0]), orow[0], olab[0],
                     classnames[olab[0]] if olab[0] >= 0 else "", float(osim[0]), int(bool(a["suspect"][i])), a["duplicate_of"][i]))
        for side, rs, ls, ss in (("in", ir, [label] * len(ir), isim), ("out", orow, olab, osim)):
            neighbours += [(row, side, j, r, l, float(v)) for j, (r, l, v) in enumerate(zip(rs, ls, ss)) if r >= 0]
    classes = [(c, classnames[c], int(shots[c]), a["class_suspects"][c], a["class_duplicates"][c]) for c in range(len(classnames))]
    return rows, neighbours, classes


def write_bank_audit(out_dir: str, tables) -> None:
    """bank_audit.csv, bank_audit_neighbours.csv and bank_audit_classes.csv in out_dir; similarities are repr(float), as the score of
    predictions.csv."""
    for name, cols, lines, floats in zip(AUDIT_FILES, (AUDIT_COLUMNS, AUDIT_NEIGHBOUR_COLUMNS, AUDIT_CLASS_COLUMNS), tables, ((5, 9), (5,), ())):
        _write_csv(osp.join(out_dir, name), cols, lines, floats)


def check_audit(args, trainer_name: str, zeroshot: bool, world=None):
    """The refusals of `--audit-bank [K]` / `--dup-threshold T`, before anything is listed or loaded (world: WORLD_SIZE, if the caller read it)."""
    if args.audit_bank is None:
        if args.dup_threshold is not None:
            raise SystemExit("--dup-threshold T belongs to --audit-bank [K]: the similarity from which a neighbour counts as a duplicate")
        return
    if zeroshot:
        raise SystemExit(f"--audit-bank: --trainer {trainer_name} has no exemplars to audit (MM_CLS_OP only; a zero-shot trainer's classifier rows are text features)")
    if args.classifiers:
        raise SystemExit(f"--audit-bank: --classifiers {args.classifiers!r} holds no exemplar features (generate in this run, or start from --bank)")
    if not 1 <= args.audit_bank <= MAX_NEAREST:
        raise SystemExit(f"--audit-bank {args.audit_bank}: K must lie in [1, {MAX_NEAREST}]")
    if args.dup_threshold is not None and args.dup_threshold != args.dup_threshold:
        raise SystemExit("--dup-threshold nan: T must be a number")
    if (int(os.environ.get("WORLD_SIZE", "1")) if world is None else world) > 1:
        raise SystemExit("--audit-bank runs in one process: a sharded rank holds only its own classes' exemplar features")


PROBE_TRAINER = "LinearProbe"
DEFAULT_PROBE_STEPS = 8


def check_probe(args, trainer_name: str):
    """The refusals of `--probe-c VALUE | search`, `--probe-val-split NAME`, `--probe-steps N` and `--probe FILE`, before anything is listed
    or loaded -> (c: a float, "search", or None under --probe FILE; steps), or (None, None) for another trainer."""
    import math
    if trainer_name != PROBE_TRAINER:
        for flag, v in (("--probe-c", args.probe_c), ("--probe-val-split", args.probe_val_split), ("--probe-steps", args.probe_steps),
                        ("--probe", args.probe or None)):
            if v is not None:
                raise SystemExit(f"{flag} belongs to --trainer {PROBE_TRAINER}: the logistic regression on the exemplars' image features")
        return None, None
    if args.probe and args.probe_c is not None:
        raise SystemExit("--probe FILE installs a fitted probe: not together with --probe-c, which fits one")
    search = args.probe_c == "search"
    if args.probe_steps is not None and not search:
        raise SystemExit("--probe-steps N belongs to --probe-c search: the rounds of its left / right comparison")
    if args.probe_val_split is not None and not search:
        raise SystemExit("--probe-val-split NAME belongs to --probe-c search: the split that scores its candidates")
    if search and not args.probe_val_split:
        raise SystemExit("--probe-c search needs --probe-val-split NAME: the split that scores its candidates")
    if args.nearest is not None or args.audit_bank is not None:
        raise SystemExit(f"--nearest / --audit-bank: --trainer {PROBE_TRAINER} keeps no exemplar features to search (MM_CLS_OP only)")
    for flag, on in (("--save-bank", args.save_bank), ("--classifiers", args.classifiers),
                     ("--add-classes / --replace-classes / --remove-classes", args.add_classes or args.replace_classes or args.remove_classes),
                     ("--ragged-shots", args.ragged_shots)):
        if on:
            raise SystemExit(f"{flag}: --trainer {PROBE_TRAINER} generates no vocabulary (MM_CLS_OP only)")
    if args.probe and args.bank:
        raise SystemExit("--probe FILE installs a fitted probe: not together with --bank, which is fitted from")
    if args.probe and not osp.isfile(args.probe):
        raise SystemExit(f"--probe {args.probe!r}: no such file")
    if args.probe:
        return None, None
    if search:
        steps = DEFAULT_PROBE_STEPS if args.probe_steps is None else args.probe_steps
        if not 0 <= steps <= 64:
            raise SystemExit(f"--probe-steps {steps}: N must lie in [0, 64]")
        if args.bank:
            raise SystemExit("--probe-c search fits on the exemplars of --root: not together with --bank")
        return "search", steps
    try:
        c = 1.0 if args.probe_c is None else float(args.probe_c)
    except ValueError:
        c = float("nan")
    if not (math.isfinite(c) and c > 0):
        raise SystemExit(f"--probe-c {args.probe_c}: VALUE must be a positive number, or `search`")
    return c, None


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    # the reference's flags, with the reference's defaults (train.py:183-255)
    ap.add_argument("--root", type=str, default="", help="path to dataset")
    ap.add_argument("--output-dir", type=str, default="", help="output directory")
    ap.add_argument("--resume", type=str, default="")
    ap.add_argument("--seed", type=int, default=-1, help="only positive value enables a fixed seed")
    ap.add_argument("--config-file", type=str, default="", help="path to config file")
    ap.add_argument("--dataset-config-file", type=str, default="", help="path to config file for dataset setup")
    ap.add_argument("--init_weight", type=str, default="")
    ap.add_argument("--trainer", type=str, default="", help="name of trainer")
    ap.add_argument("--backbone", type=str, default="", help="name of CNN backbone")
    ap.add_argument("--eval-only", action="store_true", help="evaluation only")
    ap.add_argument("--model-dir", type=str, default="", help="load model from this directory for eval-only mode.  A checkpoint written by the "
                    "reference's save_checkpoint also pickles scheduler / optimiser objects: it is read with a restricted unpickler (tensors load, the "
                    "objects become inert placeholders, no code from the file runs); OVMR_TRUSTED_CHECKPOINTS=1 asks for torch's full unpickling instead")
    ap.add_argument("--load-epoch", type=int, help="load model weights at this epoch for evaluation")
    ap.add_argument("--eval_tau", type=float)
    ap.add_argument("--eval_mode", type=str, default="multimodal")
    ap.add_argument("--n_ctx", type=int, help="number of ctx")
    ap.add_argument("--no-train", action="store_true")
    # flags of train.py the generation / evaluation modes never read (DA / DG domains, training augmentations, the stage-1 classifier,
    # head and stage number): accepted so that a reference command line runs unchanged, and ignored
    ap.add_argument("--source-domains", type=str, nargs="+", help="(accepted, ignored)")
    ap.add_argument("--target-domains", type=str, nargs="+", help="(accepted, ignored)")
    ap.add_argument("--transforms", type=str, nargs="+", help="INPUT.TRANSFORMS (train.py:69-70): of the test transform only `normalize` depends on it")
    ap.add_argument("--fs_classifier", type=str, default="", help="(accepted, ignored)")
    ap.add_argument("--head", type=str, default="", help="(accepted, ignored)")
    ap.add_argument("--stage_num", type=int, help="(accepted, ignored)")
    ap.add_argument("--visual_token_path", type=str, default="visual token path", help="(accepted, ignored)")
    # this runner's own
    ap.add_argument("--clip-weights", required=True, help="OpenAI CLIP .pt (TorchScript archive or state dict); the reference downloads it by MODEL.BACKBONE.NAME")
    ap.add_argument("--bpe-path", default=os.environ.get("OVMR_BPE_PATH"))
    ap.add_argument("--eval-split", default="train")
    ap.add_argument("--test-split", default="val")
    ap.add_argument("--exemplar-list", default="", help="text file, one `<image path> <label>` per line: use exactly these exemplars (e.g. a "
                    "reference run's few-shot set) instead of drawing NUM_SHOTS per class under --seed; labels are those BEFORE class subsampling")
    ap.add_argument("--ragged-shots", action="store_true", help="every class uses exactly the exemplars it has: min(available, DATASET.NUM_SHOTS) "
                    "images, drawn as without the flag, and NO filling of short classes with duplicates; with --exemplar-list the listed rows as "
                    "they are (1 to NUM_SHOTS per class).  A class without any exemplar is an error that names it")
    ap.add_argument("--predict", metavar="PATH", default=None, help="ranked prediction on UNLABELLED images instead of the test pass: a directory "
                    "(every image file below it, sorted by path) or a text file with one image path per line; writes OUTPUT_DIR/predictions.csv")
    ap.add_argument("--topk", type=int, default=None, metavar="K", help="classes per image of --predict, best first (default 5; 1 <= K <= min(32, classes))")
    ap.add_argument("--retrieve", metavar="PATH", default=None, help="search an UNLABELLED image pool by class instead of the test pass: PATH is listed "
                    "as --predict lists it; writes OUTPUT_DIR/retrieval.csv (label,classname,rank,image,score: the --per-class best images of "
                    "every class, best first, equal scores to the image listed first).  Any of the three trainers, after a generation, from "
                    "--classifiers FILE or from --bank FILE (no --root needed); under torch.distributed.run the pool's batches are sharded over "
                    "the ranks and rank 0 writes the one-process file")
    ap.add_argument("--per-class", type=int, default=None, metavar="M", help="images per class of --retrieve (default 32; 1 <= M <= 32)")
    ap.add_argument("--within-top", type=int, default=None, metavar="K", help="with --retrieve: search a class only among the images that rank it "
                    "within their K best scores, ties at the cut included (1 <= K <= min(32, classes); default: among all images)")
    ap.add_argument("--nearest", type=int, default=None, metavar="N", help="with --predict --trainer MM_CLS_OP: also write OUTPUT_DIR/neighbours.csv, the N "
                    "nearest exemplars of every (image, predicted class) (1 <= N <= 32; after a generation in this run, or from --bank)")
    ap.add_argument("--audit-bank", type=int, nargs="?", const=5, default=None, metavar="K", help="MM_CLS_OP: audit the exemplar features -- every "
                    "exemplar's K (default 5; 1 <= K <= 32) nearest neighbours inside its class (itself left out) and outside it -- and write "
                    "OUTPUT_DIR/bank_audit.csv (one line per exemplar: `suspect` = the closest image of another class is strictly closer than the "
                    "closest class-mate; `duplicate_of` = the best neighbour where its similarity reaches --dup-threshold), bank_audit_neighbours.csv "
                    "and bank_audit_classes.csv.  From --bank FILE without --predict or an edit nothing else runs: nothing is decoded or encoded "
                    "and no --root is needed; otherwise the audit runs on the state at the end of the generation or the edit, before --predict "
                    "or the test pass")
    ap.add_argument("--dup-threshold", type=float, default=None, metavar="T", help="with --audit-bank: a neighbour of similarity >= T is reported as a "
                    "duplicate (default 0.995: an fp16 L2-normalised feature scores a byte-identical copy at least 0.9990, so copies are always "
                    "found; re-compressed near-duplicates need a lower value, which nobody has measured on real images)")
    ap.add_argument("--classifiers", metavar="FILE", default="", help="with --predict --trainer MM_CLS_OP: load this mm_classifiers.pt instead of "
                    "generating the classifiers (no exemplar is decoded, no model file is written)")
    ap.add_argument("--save-bank", action="store_true", help="MM_CLS_OP generation: also write OUTPUT_DIR/reference_bank.pt (ovmr_amd/bank.py), "
                    "the state a later --bank run starts from; one process only")
    ap.add_argument("--bank", metavar="FILE", default="", help="MM_CLS_OP: start from this reference bank instead of generating (no exemplar is "
                    "decoded; with --predict no --root is needed)")
    ap.add_argument("--add-classes", metavar="DIR", default="", help="with --bank: append the classes of DIR (one sub-folder of images per class, "
                    "sorted; names from DIR/classnames.txt, else the folder name)")
    ap.add_argument("--replace-classes", metavar="DIR", default="", help="with --bank: new exemplars for existing classes (layout as --add-classes; "
                    "every folder must name a class of the bank)")
    ap.add_argument("--remove-classes", metavar="NAME", nargs="+", default=None, help="with --bank: drop these classes (edits apply in the order "
                    "remove, replace, add)")
    ap.add_argument("--per-class-result", action="store_true", help="the test pass also prints the reference's `=> per-class result` block and "
                    "reports perclass_accuracy (the reference's TEST.PER_CLASS_RESULT; counted on the GPU by ovmr_eval_detail)")
    ap.add_argument("--confusion-matrix", action="store_true", help="the test pass also writes OUTPUT_DIR/cmat.pt, the row-normalised confusion "
                    "matrix (the reference's TEST.COMPUTE_CMAT; counted on the GPU by ovmr_eval_detail)")
    ap.add_argument("--score-curves", type=int, nargs="?", const=DEFAULT_BINS, default=None, metavar="BINS", help="the test pass also keeps, per "
                    "class, the histograms of the scores of its own images and of all others (BINS bins, default 256, at most 4096), reports "
                    "mAP and mean AUROC and writes OUTPUT_DIR/curves_per_class.csv and score_hist.pt (per mode under --eval_mode all)")
    ap.add_argument("--score-range", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="with --score-curves: the scores the bins "
                    "cover (default 0 1 for MM_CLS_OP's probabilities; required for the zero-shot trainers' logits)")
    ap.add_argument("--exact-curves", action="store_true", help="the test pass also keeps every score on the GPU and, when it ends, counts "
                    "them against each class's own positive scores (ovmr_eval_ranks): reports exact_mAP and exact_mean_auroc -- the figures "
                    "sklearn gives on the raw scores, from any trainer, no range needed -- and writes OUTPUT_DIR/ranks_per_class.csv and "
                    "rank_state.pt (per mode under --eval_mode all)")
    ap.add_argument("--exact-budget", type=float, default=None, metavar="GIB", help="with --exact-curves: the most memory the kept scores may "
                    "take, in GiB (default 16; 50 000 images x 1000 classes are 0.2 GiB in fp32); the batch that would pass it ends the run")
    ap.add_argument("--probe-c", default=None, metavar="VALUE", help="--trainer LinearProbe: the strength C of the logistic regression fitted on the "
                    "exemplars' image features (scikit-learn's C; default 1.0), or `search`: the reference's search of C against "
                    "--probe-val-split (lpclip/linear_probe.py)")
    ap.add_argument("--probe-val-split", default=None, metavar="NAME", help="with --probe-c search: the split whose images score the candidates; "
                    "min(NUM_SHOTS, 4) images per class of it (the reference's table), drawn with the job's seed, encoded once")
    ap.add_argument("--probe-steps", type=int, default=None, metavar="N", help="with --probe-c search: rounds of left / right comparison after the "
                    "7-point sweep (default 8)")
    ap.add_argument("--probe", metavar="FILE", default="", help="--trainer LinearProbe: install this linear_probe.pt and fit nothing; with --predict / "
                    "--retrieve the class names come from the file and no --root is needed.  (--bank FILE with this trainer fits from the "
                    "bank's features and shots instead of decoding exemplars; the bank is held to the model by embed_dim only)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--workers", type=int, default=None,
                    help="decode worker processes of the pipelined loader (default: DATALOADER.NUM_WORKERS); 0 = decode in this thread")
    ap.add_argument("--prefetch", type=int, default=3, help="batches the workers decode ahead")
    ap.add_argument("--host-resize", action="store_true", help="Resize + CenterCrop in the decode workers (PIL) instead of on the GPU (ovmr_resize_crop_u8; same bytes either way)")
    ap.add_argument("--fast-decode", action="store_true", help="JPEG draft mode (DCT-domain downscale): faster, pixels differ slightly from the reference's")
    ap.add_argument("opts", default=None, nargs=argparse.REMAINDER, help="modify config options using the command-line (KEY VALUE pairs)")
    return ap.parse_args(argv)


def build_splits(cfg, eval_split: str = "train", test_split: str = "val", exemplar_list: str = "", ragged: bool = False):
    """What the reference's dataset class hands the DataManager (datasets/imagenet.py:16-64), for a folder dataset: the few-shot
    draw of `eval_split` under cfg.SEED (or the images listed in `exemplar_list`), THEN the class subsampling of
    DATASET.SUBSAMPLE_CLASSES applied to the exemplar and the test items alike (:60-62), the class names of the surviving labels in
    label order.  Returns (classnames, exemplar items laid out NUM_SHOTS rows per class, test items); with `ragged` the exemplar items
    are every class's own rows, unfilled (layout_exemplars_ragged)."""
    from . import config
    shots, seed, sub = cfg.DATASET.NUM_SHOTS, cfg.SEED, cfg.DATASET.SUBSAMPLE_CLASSES
    root = cfg.DATASET.ROOT
    folders, eval_all = list_split(root, eval_split)
    all_names = read_classnames(root, folders)
    test_items = list_split(root, test_split)[1] if test_split else []       # (a prediction run has no labelled test split)
    if exemplar_list:
        few = read_exemplar_list(exemplar_list, len(folders), shots)
    else:
        few = fewshot_items(eval_all, shots, seed)
    if ragged:
        missing = sorted(set(range(len(folders))) - {l for _, l in few})
        if missing:
            raise SystemExit("no exemplar image for class " + ", ".join(f"{all_names[y]!r} (folder {folders[y]!r})" for y in missing[:8])
                             + (f" and {len(missing) - 8} more" if len(missing) > 8 else ""))
    all_labels = sorted({l for _, l in few})                  # the label set `subsample_classes` splits (train_x, oxford_pets.py:160-168)
    few, test_items = config.subsample_classes(few, test_items, subsample=sub)
    half = -(-len(all_labels) // 2)
    kept = {"all": all_labels, "base": all_labels[:half], "new": all_labels[half:]}[sub]
    if sub == "all" and kept != list(range(len(folders))):
        raise SystemExit(f"{len(folders) - len(kept)} class folder(s) of {eval_split!r} hold no exemplar image")
    classnames = [all_names[y] for y in kept]                 # lab2cname of the relabelled train_x (base_dataset.py get_lab2cname)
    return classnames, layout_exemplars_ragged(few, shots) if ragged else layout_exemplars(few, shots, seed), test_items


def list_edit_classes(directory: str, shots: int, seed: int, ragged: bool = False, flag: str = "--add-classes"):
    """The classes of an `--add-classes` / `--replace-classes` folder: one sub-folder of images per class, sorted folder order = the
    loader's labels 0 ... K - 1; names from DIR/classnames.txt (read_classnames), else the folder name.  Every class's exemplars are drawn
    with fewshot_items and laid out with layout_exemplars (or layout_exemplars_ragged), under `seed` and `shots`, exactly as build_splits
    does for a data set.  Returns (class names, exemplar items in loader order)."""
    if not osp.isdir(directory):
        raise SystemExit(f"{flag} {directory!r}: no such directory")
    folders = sorted(f.name for f in os.scandir(directory) if f.is_dir() and not f.name.startswith("."))
    if not folders:
        raise SystemExit(f"{flag} {directory!r}: no class folder below this directory")
    items = []
    for label, folder in enumerate(folders):
        names = sorted(n for n in os.listdir(osp.join(directory, folder)) if not n.startswith("."))
        if not names:
            raise SystemExit(f"{flag} {directory!r}: class folder {folder!r} holds no image")
        items += [(osp.join(directory, folder, n), label) for n in names]
    few = fewshot_items(items, shots, seed)
    return read_classnames(directory, folders), layout_exemplars_ragged(few, shots) if ragged else layout_exemplars(few, shots, seed)


def plan_vocabulary_edits(args, bank_names: Sequence[str], shots: int, seed: int, ragged: bool):
    """What `--remove-classes / --replace-classes / --add-classes` ask for, checked against the bank's class names before the model
    exists: ([names to remove], (names, items) to replace or None, (names, items) to add or None, the final class names)."""
    names = list(bank_names)
    remove = list(args.remove_classes or [])
    for n in remove:
        if n not in names:
            raise SystemExit(f"--remove-classes: the bank has no class {n!r}")
        if remove.count(n) > 1:
            raise SystemExit(f"--remove-classes: class {n!r} is named twice")
    names = [n for n in names if n not in remove]
    if not names:
        raise SystemExit("--remove-classes: removing every class leaves no vocabulary")
    replace = add = None
    if args.replace_classes:
        replace = list_edit_classes(args.replace_classes, shots, seed, ragged, "--replace-classes")
        for n in replace[0]:
            if n not in names:
                raise SystemExit(f"--replace-classes {args.replace_classes!r}: the bank has no class {n!r}"
                                 + (" left (it is removed in the same run)" if n in remove else ""))
    if args.add_classes:
        add = list_edit_classes(args.add_classes, shots, seed, ragged, "--add-classes")
        for n in add[0]:
            if n in names or add[0].count(n) > 1:
                raise SystemExit(f"--add-classes {args.add_classes!r}: class {n!r} is in the vocabulary already")
        names = names + list(add[0])
    return remove, replace, add, names


def _label_order_paths(items):
    """The paths of exemplar items class after class in label order, a class's rows in loader order: the rows of a bank's `features`."""
    return [p for p, _ in sorted(items, key=lambda it: it[1])]


def _paths_per_class(items, K: int):
    per = [[] for _ in range(K)]
    for p, l in items:
        per[l].append(p)
    return per


BACKBONES = {"ViT-B/16": (768, 16, 12), "ViT-B/32": (768, 32, 12), "ViT-L/14": (1024, 14, 24), "ViT-L/14@336px": (1024, 14, 24)}   # clip/clip.py:32-40 (ViT entries)


def _check_model_matches_cfg(spec, cfg) -> None:
    name, size = cfg.MODEL.BACKBONE.NAME, spec.image_resolution
    if name:
        if name not in BACKBONES:
            raise SystemExit(f"MODEL.BACKBONE.NAME {name!r}: only the ViT CLIP models are on the hot path ({sorted(BACKBONES)})")
        if (spec.vision_width, spec.vision_patch_size, spec.vision_layers) != BACKBONES[name]:
            raise SystemExit(f"--clip-weights holds a ViT of width {spec.vision_width}, patch {spec.vision_patch_size}, {spec.vision_layers} layers: "
                             f"not MODEL.BACKBONE.NAME {name!r}")
    if tuple(cfg.INPUT.SIZE) != (size, size):
        raise SystemExit(f"INPUT.SIZE {tuple(cfg.INPUT.SIZE)} does not match the model's input resolution {size} "
                         "(the positional embedding has one row per patch of that resolution, clip/model.py:416)")


def _init_process_group(args) -> bool:
    """Launched by torch.distributed.run (scripts/generate_classifier.sh / eval_ovmr.sh with several GPUs): one rank per GPU, process group
    nccl = RCCL; forward_prompt then shards the classes over the ranks (two collectives), every rank evaluates its own
    batches of the test set, the evaluator state is summed over the ranks and rank 0 reports and writes.
    True when the group was opened here (and is this runner's to close); `args.device` becomes the rank's own GPU."""
    import torch
    import torch.distributed as dist
    own_group = False
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and not dist.is_initialized():
        if "RANK" not in os.environ:
            raise SystemExit(f"WORLD_SIZE is {os.environ['WORLD_SIZE']} but RANK is not set: a job over several ranks is one process per GPU, "
                             "each with its own RANK (torch.distributed.run sets them: scripts/eval_ovmr.sh)")
        local = int(os.environ.get("LOCAL_RANK", "0"))
        backend = os.environ.get("OVMR_DIST_BACKEND", "nccl")
        if backend == "nccl":
            args.device = f"cuda:{local}"
        torch.cuda.set_device(torch.device(args.device))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # a rank reaches the sum of the evaluator state, and the closing barrier, when ITS batches of the test pass are done, and waits there
        # for the slowest rank: the collective timeout has to cover the skew between ranks over a test pass (a slower GPU, a cold page cache,
        # one batch more), which nobody has measured -- it stays sized for a whole pass, not for a collective (the backend's default of 10
        # minutes would abort the waiting ranks, and the launcher then the others)
        import datetime
        to = datetime.timedelta(seconds=float(os.environ.get("OVMR_DIST_TIMEOUT", 6 * 3600)))
        dist.init_process_group(backend, timeout=to, **({"device_id": torch.device(args.device)} if backend == "nccl" else {}))
        own_group = True
    return own_group


def _loader_factory(args, cfg, size: int, tfm: dict):
    """loader(items, batch, rank, world, n_classes, ragged=, batch_shard=): the pipelined loader, or with no decode workers the in-thread
    FolderLoader."""
    workers = cfg.DATALOADER.NUM_WORKERS if args.workers is None else args.workers
    cls, kw = FolderLoader, tfm
    if workers > 0:
        from .loader import PipelinedFolderLoader as cls
        kw = dict(workers=workers, prefetch=args.prefetch, device=args.device, fast_decode=args.fast_decode, device_resize=not args.host_resize, **tfm)
    return lambda items, batch, rank=0, world=1, n_classes=0, ragged=False, batch_shard=None: cls(
        items, batch, size, rank, world, n_classes, ragged=ragged, batch_shard=batch_shard, **kw)


def _report_pipeline(results: dict, name: str, loader) -> None:
    st = getattr(loader, "stats", None)      # (a FolderLoader keeps none)
    if st:
        print(f"input pipeline, {name}: {st['images']} images in {st['wall_s']:.2f} s = {st['images_per_s']:.0f} img/s end to end "
              f"({st['workers']} decode workers, {st.get('device_resized', 0)} images resized on the GPU / {st.get('host_resized', 0)} by the workers), "
              f"host blocked on decode {st['decode_wait_s']:.2f} s = {100 * st['decode_bound_fraction']:.0f} % of the time")
        results[f"pipeline_{name.split()[0]}"] = st


def plan_job(args, cfg):
    """Stage 1, before torch is imported: every refusal that needs neither a process group, a bank's contents nor the data set, in the
    order a user meets them, then what the job is, as one record for the stages (the fields: the SimpleNamespace below).  mode "audit" is
    the bank's audit and nothing else; lift_shots: no exemplar of the data set is decoded, so its class list (the label set of the few-shot
    draw) is drawn with NUM_SHOTS >= 1 whatever the configuration says; skip: the job would write mm_classifiers.pt where one exists."""
    from . import templates
    name = cfg.TRAINER.NAME
    zeroshot = name in templates.ZEROSHOT_TRAINERS
    probe = name == PROBE_TRAINER
    if not (zeroshot or probe or name == "MM_CLS_OP") or not args.eval_only:
        raise SystemExit("only `--eval-only --trainer MM_CLS_OP` (classifier generation / evaluation) and `--eval-only --trainer "
                         "ZeroshotCLIP | ZeroshotCLIP2` (zero-shot evaluation) are on the hot path")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    shots, batch = cfg.DATASET.NUM_SHOTS, cfg.DATALOADER.TEST.BATCH_SIZE
    probe_c, probe_steps = check_probe(args, name)
    logits = zeroshot or probe                                # [B, C] scores whatever EVAL_MODE says, and no natural range
    edits = bool(args.add_classes or args.replace_classes or args.remove_classes)
    if edits and not args.bank:
        raise SystemExit("--add-classes / --replace-classes / --remove-classes edit a reference bank: give --bank FILE")
    if zeroshot and (args.bank or args.save_bank):
        raise SystemExit(f"--bank / --save-bank: --trainer {name} has no generated vocabulary to bank (MM_CLS_OP only; a zero-shot "
                         "vocabulary is a text call away)")
    if (args.bank or args.save_bank) and world > 1:
        raise SystemExit("--bank / --save-bank run in one process: a sharded rank holds only its own classes' exemplar features")
    if args.bank and args.save_bank:
        raise SystemExit("--save-bank belongs to a generation job: a --bank run writes OUTPUT_DIR/reference_bank.pt whenever it edits")
    if args.bank and args.classifiers:
        raise SystemExit("--bank holds the classifiers already: not together with --classifiers")
    if args.bank and not osp.isfile(args.bank):
        raise SystemExit(f"--bank {args.bank!r}: no such file")
    predict, retrieve = args.predict is not None, args.retrieve is not None
    check_retrieve(args, name, logits, cfg.EVAL_MODE)
    pool = predict or retrieve                                # unlabelled images instead of the labelled test split
    curve_bins, curve_range = check_score_curves(args, name, logits)
    exact, exact_bytes = check_exact_curves(args)
    check_nearest(args, name, zeroshot)
    check_audit(args, name, zeroshot, world)
    images, k, m = [], None, (MAX_PER_CLASS if args.per_class is None else args.per_class) if retrieve else None
    if predict:
        if cfg.EVAL_MODE == "all" and not logits:
            raise SystemExit("--predict ranks the classes under ONE mode: --eval_mode all belongs to the test pass (fusion, text, vision or multimodal here)")
        for flag, on in (("--per-class-result", args.per_class_result), ("--confusion-matrix", args.confusion_matrix)):
            if on:
                raise SystemExit(f"{flag} belongs to the test pass: --predict ranks unlabelled images, there is nothing to count")
        if world > 1:
            raise SystemExit(PREDICT_ONE_PROCESS)
        k = 5 if args.topk is None else args.topk
        if not 1 <= k <= MAX_TOPK:
            raise SystemExit(f"--topk {k}: K must lie in [1, min({MAX_TOPK}, number of classes)]")
    if pool:
        if args.classifiers and zeroshot:
            raise SystemExit(f"--classifiers {args.classifiers!r}: --trainer {name} has no generated classifiers to load (MM_CLS_OP only)")
        if args.classifiers and not osp.isfile(args.classifiers):
            raise SystemExit(f"--classifiers {args.classifiers!r}: no such file")
        images = list_predict_images(args.predict, "--predict") if predict else list_predict_images(args.retrieve, "--retrieve")
        if retrieve:
            check_pool_size(len(images), args.retrieve)
    elif args.topk is not None or args.classifiers:
        raise SystemExit("--topk / --classifiers belong to --predict PATH (the test pass takes TEST.TOPK)")
    vocabulary = ("probe-file" if args.probe else "probe-bank" if args.bank else "probe-fit") if probe else "zeroshot" if zeroshot else "classifiers" if args.classifiers else "bank" if args.bank else "generate"
    audit_only = args.audit_bank is not None and vocabulary == "bank" and not edits and not pool      # the bank alone: no data set, no test pass
    p = SimpleNamespace(args=args, cfg=cfg, zeroshot=zeroshot, world=world, vocabulary=vocabulary, edits=edits, images=images,
                        mode="audit" if audit_only else "predict" if predict else "retrieve" if retrieve else "test",
                        k=k, m=m, within_top=args.within_top, nearest=args.nearest, audit=args.audit_bank,
                        dup_threshold=0.995 if args.dup_threshold is None else args.dup_threshold, curve_bins=curve_bins, curve_range=curve_range,
                        exact=exact, exact_bytes=exact_bytes, probe=probe, probe_c=probe_c, probe_steps=probe_steps,
                        ragged=bool(args.ragged_shots) and vocabulary in ("generate", "bank"), lift_shots=vocabulary not in ("generate", "probe-fit"), skip=False)
    decodes = vocabulary == "generate" or edits               # exemplars are decoded and mm_classifiers.pt is written
    if decodes and osp.isdir(cfg.OUTPUT_DIR) and osp.exists(osp.join(cfg.OUTPUT_DIR, "mm_classifiers.pt")):
        p.skip = True
        return p
    if zeroshot:
        try:
            templates.check_dataset(cfg.DATASET.NAME)
        except KeyError as e:
            raise SystemExit(e.args[0]) from None
        # (nothing of the few-shot draw is decoded)
    elif decodes or vocabulary == "probe-fit":
        if shots < 1:
            raise SystemExit("DATASET.NUM_SHOTS must be >= 1: the eval-set loader draws NUM_SHOTS rows per class (data_manager.py:157-170)")
        if batch < shots:
            raise SystemExit(f"DATALOADER.TEST.BATCH_SIZE {batch} is smaller than DATASET.NUM_SHOTS {shots}: a loader batch holds whole classes "
                             f"(RandomClassSampler needs one class per batch), raise TEST.BATCH_SIZE to at least {shots}")
        if cfg.DATALOADER.K_TRANSFORMS != 1:
            raise SystemExit("DATALOADER.K_TRANSFORMS > 1 only applies to training transforms; the test transform has one view")
    return p


def _open_job(p):
    """Stage 2: the process group, the seed, the bank and the edits it is asked for, the splits -> the job's state (rank, world,
    own_group, bank, edit_plan, classnames, exemplars, test_items).  The refusals that need one of these stand here."""
    import torch
    import torch.distributed as dist
    args, cfg, pool = p.args, p.cfg, p.mode in ("predict", "retrieve")
    own_group = _init_process_group(args)
    rank, world = (dist.get_rank(), dist.get_world_size()) if dist.is_available() and dist.is_initialized() else (0, 1)
    if p.mode == "predict" and world > 1:                     # (a group the caller opened: WORLD_SIZE > 1 was refused by the plan)
        raise SystemExit(PREDICT_ONE_PROCESS)
    if cfg.SEED >= 0:
        print(f"Setting fixed seed: {cfg.SEED}")              # train.py:157-159
        torch.manual_seed(cfg.SEED)
    split_cfg = cfg
    if p.lift_shots:
        import copy
        split_cfg = copy.deepcopy(cfg)
        split_cfg.DATASET.NUM_SHOTS = max(1, cfg.DATASET.NUM_SHOTS)          # (any NUM_SHOTS >= 1 yields the same label set)
    bank_obj = edit_plan = probe_state = None
    if p.vocabulary in ("probe-file", "probe-bank"):
        # the class names come from the file: a pool needs no data set at all, the test pass one that speaks of the same classes
        from . import bank as bank_format
        from . import probe as probe_format
        flag, path = ("--probe", args.probe) if p.vocabulary == "probe-file" else ("--bank", args.bank)
        try:
            if p.vocabulary == "probe-file":
                probe_state = probe_format.LinearProbeState.read(path)
                classnames = list(probe_state.classnames)
            else:
                bank_obj = bank_format.read(path)
                classnames = bank_obj["classnames"]
        except ValueError as e:
            raise SystemExit(str(e)) from None
        if classnames is None:
            raise SystemExit(f"--bank {path!r}: the bank holds no class names (it was written by a model built from token rows)")
        exemplars, test_items = [], []
        if p.mode == "test":
            set_names, _, test_items = build_splits(split_cfg, args.eval_split, args.test_split, "", False)
            diff = bank_format.first_difference(classnames, set_names)
            if diff is not None:
                raise SystemExit(f"{flag} {path!r}: its class names are not the data set's: {diff}")
    elif p.vocabulary == "bank":
        from . import bank as bank_format
        try:
            bank_obj = bank_format.read(args.bank)            # (checked against the model by load_bank)
        except ValueError as e:
            raise SystemExit(str(e)) from None
        if bank_obj["classnames"] is None:
            raise SystemExit(f"--bank {args.bank!r}: the bank holds no class names (it was written by a model built from token rows)")
        edit_plan = plan_vocabulary_edits(args, bank_obj["classnames"], cfg.DATASET.NUM_SHOTS, cfg.SEED, p.ragged)
        classnames, exemplars, test_items = edit_plan[3], [], []
        if p.mode == "test":                                  # the data set the test pass runs on must speak of the same classes
            set_names, _, test_items = build_splits(split_cfg, args.eval_split, args.test_split, "", False)
            diff = bank_format.first_difference(classnames, set_names)
            if diff is not None:
                raise SystemExit(f"--bank {args.bank!r}: its class names" + (" (after the edits)" if p.edits else "") + f" are not the data set's: {diff}")
    else:
        classnames, exemplars, test_items = build_splits(split_cfg, args.eval_split, None if pool else args.test_split, args.exemplar_list, p.ragged)
    for flag, v in (("--topk", p.k), ("--within-top", p.within_top)):           # (each is None without its mode)
        if v is not None and v > len(classnames):
            raise SystemExit(f"{flag} {v}: K must lie in [1, min({MAX_TOPK}, {len(classnames)} classes)]")
    if pool:
        test_items = [(path, 0) for path in p.images]         # the loader protocol carries a label: a dummy one, never read
    return SimpleNamespace(own_group=own_group, rank=rank, world=world, bank=bank_obj, edit_plan=edit_plan, classnames=classnames,
                           exemplars=exemplars, test_items=test_items, audit_tables=None, probe_state=probe_state)


def _build_trainer(p, run):
    """Stage 3: the CLIP weights, the loaders (run.eval_loader or None, run.edit_loaders, run.test_loader) and the trainer (run.tr)."""
    from . import checkpoint, modules, trainer
    from .tokenizer import BPETokenizer
    args, cfg, classnames, rank, world = p.args, p.cfg, run.classnames, run.rank, run.world
    shots, batch, ragged = cfg.DATASET.NUM_SHOTS, cfg.DATALOADER.TEST.BATCH_SIZE, p.ragged
    # what the loaders need to know of the model is in the weights' shapes: the decode workers start before the engine exists
    clip_sd = checkpoint.load_clip_state_dict(args.clip_weights)
    spec = modules.infer_spec(clip_sd)
    _check_model_matches_cfg(spec, cfg)
    normalize = "normalize" in tuple(cfg.INPUT.TRANSFORMS)    # transforms.py:514-518
    tfm = dict(interpolation=cfg.INPUT.INTERPOLATION, mean=tuple(cfg.INPUT.PIXEL_MEAN) if normalize else None,
               std=tuple(cfg.INPUT.PIXEL_STD) if normalize else None)
    kw = {}
    if p.probe:
        kw["probe_c"] = p.probe_c if isinstance(p.probe_c, float) else 1.0
    elif not p.zeroshot:
        pl_state = None
        if cfg.MODEL.INIT_WEIGHTS:                            # load_pretrained_weights (trainers/mm_classifier_one_prompt.py:403-404)
            ck = checkpoint._torch_load(cfg.MODEL.INIT_WEIGHTS)
            pl_state = ck["state_dict"] if "state_dict" in ck else ck
        if args.model_dir:
            pl_state = checkpoint.load_prompt_learner_state(args.model_dir, args.load_epoch)
        else:
            print("Note that load_model() is skipped as no pretrained model is given")       # :464-466
        kw["prompt_learner_state"] = pl_state
    loader = _loader_factory(args, cfg, spec.image_resolution, tfm)
    eval_loader, edit_loaders = None, {}
    val_loader = None
    if p.vocabulary == "probe-fit":
        # every rank decodes every exemplar and fits the same probe (the fit is not sharded: DESIGN.md section 5)
        eval_loader = loader(run.exemplars, batch // shots * shots, 0, 1, len(classnames))     # (MM_CLS_OP's batches: the same features, bit for bit)
        if p.probe_c == "search":
            from .probe import val_shots
            if cfg.DATASET.SUBSAMPLE_CLASSES != "all":
                raise SystemExit("--probe-c search scores on the classes of --probe-val-split: DATASET.SUBSAMPLE_CLASSES must be all")
            if not osp.isdir(osp.join(cfg.DATASET.ROOT, args.probe_val_split)):
                raise SystemExit(f"--probe-val-split {args.probe_val_split!r}: no such split below {cfg.DATASET.ROOT!r}")
            val_items = fewshot_items(list_split(cfg.DATASET.ROOT, args.probe_val_split)[1], val_shots(shots), cfg.SEED)
            if not val_items or max(l for _, l in val_items) >= len(classnames):
                raise SystemExit(f"--probe-val-split {args.probe_val_split!r}: its class folders are not the {len(classnames)} classes of {args.eval_split!r}")
            val_loader = loader(val_items, batch, 0, 1, len(classnames))
    elif p.vocabulary == "generate" and not ragged:
        eval_loader = loader(run.exemplars, batch // shots * shots, rank, world, len(classnames))
    else:                                                     # (zero-shot, --classifiers: no exemplar loader at all)
        try:
            if p.vocabulary == "generate":
                eval_loader = loader(run.exemplars, batch, rank, world, len(classnames), ragged=True)
            for key, part in (("replace", run.edit_plan[1]), ("add", run.edit_plan[2])) if p.vocabulary == "bank" else ():
                if part is not None:                          # the loaders of the edited classes only: nothing of an old class is listed
                    edit_loaders[key] = loader(part[1], batch if ragged else batch // shots * shots, 0, 1, len(part[0]), ragged=ragged)
        except ValueError as e:
            raise SystemExit(str(e)) from None
        if eval_loader is not None:
            n = np.sort(eval_loader.shots.numpy())
            print(f"ragged exemplar set: {int(n.sum()):,} images of {len(n):,} classes, shots per class min {int(n[0])} / median {float(np.median(n)):g} / max {int(n[-1])}")
    # the test pass is sharded by batches: every rank evaluates its contiguous range of the one-process pass's batches (shard.shard_test_batches)
    test_loader = loader(run.test_items, batch, batch_shard=(rank, world) if world > 1 else None)
    # the decode workers start while the engine takes the weights; one ring, sized for the larger batch, serves both loaders of a rank
    # (a rank whose share of the test batches is empty decodes exemplars alone: its ring is sized for those)
    first = eval_loader if eval_loader is not None and (len(test_loader) == 0 or eval_loader.bs > test_loader.bs) else test_loader
    for ld in edit_loaders.values():                          # (an edit's loader may be the one that needs the larger ring)
        if len(first) == 0 or ld.bs > first.bs:
            first = ld
    if hasattr(first, "warm"):
        first.warm()
    dm = SimpleNamespace(dataset=SimpleNamespace(classnames=classnames), test_loader=test_loader, val_loader=None, eval_set_loader=eval_loader)
    run.tr = trainer.build_trainer(cfg, dm, clip_weights=clip_sd, tokenizer=BPETokenizer(args.bpe_path), device=args.device,
                                   reserve=(batch, 256, max(1024, len(classnames))), per_class_result=args.per_class_result,
                                   compute_cmat=args.confusion_matrix, score_curves=p.curve_bins, score_range=p.curve_range,
                                   exact_curves=p.exact, exact_max_bytes=p.exact_bytes, **kw)
    run.eval_loader, run.edit_loaders, run.test_loader, run.val_loader = eval_loader, edit_loaders, test_loader, val_loader


def _install_vocabulary(p, run):
    """Stage 4: the model's classifiers -- loaded from --classifiers, taken from --bank and edited (and then saved), or generated from the
    exemplar set (and banked under --save-bank).  A zero-shot model has its text classifier already."""
    from .bank import BANK_FILE
    args, cfg, model = p.args, p.cfg, run.tr.model
    if p.probe:
        # the probe: read from --probe, fitted from --bank's features, or fitted (at --probe-c, or searched) from the exemplar loader;
        # every fit writes OUTPUT_DIR/linear_probe.pt and one `=> linear probe:` line behind the test pass
        tr = run.tr
        try:
            if p.vocabulary == "probe-file":
                tr.model.install(run.probe_state)
                tr.probe_state = run.probe_state
            elif p.vocabulary == "probe-bank":
                if int(run.bank["features"].shape[1]) != tr.model.engine.spec.embed_dim:
                    raise ValueError(f'"{args.bank}": features are {int(run.bank["features"].shape[1])} wide, the model\'s embed_dim is '
                                     f"{tr.model.engine.spec.embed_dim}")
                tr.fit_probe(features=run.bank["features"], shots=run.bank["shots"])
            elif p.probe_c == "search":
                vx, vy = tr.model.encode_loader(run.val_loader)
                tr.search_probe(vx, vy, p.probe_steps)
            else:
                tr.fit_probe()
        except ValueError as e:
            raise SystemExit(str(e)) from None
    elif p.vocabulary == "classifiers":
        model.load_classifiers(args.classifiers)
    elif p.vocabulary == "bank":
        # (the trainer and its evaluator were built for the FINAL class names; the bank replaces the model's class list, the edits lead to it)
        try:
            model.load_bank(args.bank, run.bank)
        except ValueError as e:
            raise SystemExit(str(e)) from None
        remove, replace, add, _ = run.edit_plan
        if remove:
            model.remove_classes(remove)
        if replace is not None:
            model.replace_classes(list(replace[0]), run.edit_loaders["replace"], exemplar_paths=_paths_per_class(replace[1], len(replace[0])))
        if add is not None:
            model.add_classes(list(add[0]), run.edit_loaders["add"], exemplar_paths=_paths_per_class(add[1], len(add[0])))
        assert model.classnames == run.classnames
        if p.edits:
            model.save_classifiers()
            model.save_bank(osp.join(cfg.OUTPUT_DIR, BANK_FILE))
    elif p.vocabulary == "generate":
        # the reference does this inside the first forward (:341-342); up front it keeps the two loaders' statistics apart.  Rank 0's two
        # files are written by a worker thread while the test set runs (CustomCLIP._write_files), joined at the end of test().  The
        # classifiers are complete on every rank: each goes on to its own batches of the test set
        model.forward_prompt(run.eval_loader, wait_files=False)
        if args.save_bank:
            model.save_bank(osp.join(cfg.OUTPUT_DIR, BANK_FILE), exemplar_paths=_label_order_paths(run.exemplars))


def _run_mode(p, run) -> dict:
    """Stage 5: under --audit-bank the three tables of the state the vocabulary was left in (kept as run.audit_tables), then the mode's pass
    and its files -> the results (the audit alone has none)."""
    images, classnames, out_dir = p.images, run.classnames, p.cfg.OUTPUT_DIR
    bank_rows = lambda: run.tr.model.exemplar_rows(_label_order_paths(run.exemplars))      # the bank's own paths (after the edits), or this run's
    if p.audit is not None:
        try:
            audit = run.tr.model.audit_bank(p.audit, dup_threshold=p.dup_threshold)
        except ValueError as e:
            raise SystemExit(str(e)) from None
        run.audit_tables = tables = bank_audit_tables(audit, classnames, *bank_rows())
        write_bank_audit(out_dir, tables)
        suspects, dups = sum(r[10] for r in tables[0]), sum(r[11] >= 0 for r in tables[0])
        print(f"=> bank audit: {len(tables[0]):,} exemplars, {suspects:,} suspects in {sum(c[3] > 0 for c in tables[2]):,} classes, "
              f"{dups:,} duplicates")
        print(f"=> {', '.join(osp.join(out_dir, n) for n in AUDIT_FILES)}")
    if p.mode == "audit":
        return {}
    if p.mode == "test":
        run.tr.test()
        return dict(run.tr.results)
    if p.mode == "retrieve":
        # every rank walks its own batches of the pool and ends with the job's lists (trainer.retrieve); rank 0 writes
        values, indices = run.tr.retrieve(run.test_loader, p.m, p.within_top)
        results = {"retrieval": retrieval_rows(values, indices, images, classnames)}
        if run.rank == 0:
            out_csv = osp.join(out_dir, "retrieval.csv")
            write_retrieval(out_csv, results["retrieval"])
            filled = len({r[0] for r in results["retrieval"]})
            print(f"=> the {p.m} best of {len(images):,} images for each of {len(classnames):,} classes"
                  + (f" (within each image's top {p.within_top})" if p.within_top is not None else "")
                  + f": {len(results['retrieval']):,} lines, {filled:,} classes with an image: {out_csv}")
        return results
    if p.nearest is not None:
        values, indices, sims, rows = run.tr.predict_explained(run.test_loader, p.k, p.nearest)
    else:
        values, indices = run.tr.predict(run.test_loader, p.k)
    results = {"predictions": ranked_predictions(images, values, indices, classnames)}
    out_csv = osp.join(out_dir, "predictions.csv")
    write_predictions(out_csv, results["predictions"])
    print(f"=> top-{p.k} predictions of {len(images):,} images: {out_csv}")
    if p.nearest is not None:
        results["neighbours"] = nearest_neighbours(images, indices, sims, rows, classnames, bank_rows()[1])
        out_csv = osp.join(out_dir, "neighbours.csv")
        write_neighbours(out_csv, results["neighbours"])
        print(f"=> the {p.nearest} nearest exemplars of every predicted class: {out_csv}")
    return results


def _close_job(p, run, results: dict) -> dict:
    """Stage 6: the loaders' reports, what every job's results carry, and the end of a process group opened here."""
    if run.eval_loader is not None:
        _report_pipeline(results, "exemplar set", run.eval_loader)
    for key, ld in run.edit_loaders.items():
        _report_pipeline(results, f"{key} set", ld)
    if p.mode != "audit":
        _report_pipeline(results, f"{p.mode} set", run.test_loader)
    if run.audit_tables is not None:
        results["bank_audit"] = dict(zip(("exemplars", "neighbours", "classes"), run.audit_tables))
    results["classnames"] = run.classnames
    if run.test_loader.batch_shard is not None:
        results["test_shard"] = {"rank": run.rank, "world": run.world, "batches": list(run.test_loader.batch_range), "images": len(run.test_loader.items)}
    if run.own_group:                            # (a rank that raised inside the pass never gets here: its peers end at the group's timeout)
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return results


def main(argv=None) -> Dict[str, float]:
    """train.py:183-255 on the evaluation path: build_trainer(cfg) and test().  MM_CLS_OP generates the classifiers from the exemplar set,
    writes mm_classifiers.pt / visual_tokens.pt and evaluates the test set; the zero-shot trainers take the classes and test items of the
    same job (build_splits; no exemplar is decoded) and the text classifier from DATASET.NAME's template(s), and write no model file.
    The result block and acc_per_class.csv / f1_per_class.csv land in OUTPUT_DIR; --per-class-result adds the per-class block and
    results["perclass_accuracy"], --confusion-matrix adds OUTPUT_DIR/cmat.pt, --score-curves adds two result lines, results["mAP"] /
    ["mean_auroc"], curves_per_class.csv and score_hist.pt, --exact-curves two more, results["exact_mAP"] / ["exact_mean_auroc"],
    ranks_per_class.csv and rank_state.pt."""
    from . import config
    args = parse(argv)
    p = plan_job(args, config.setup_cfg(args))                # train.py:134-155; nothing below the plan runs for a refused job
    if p.skip:
        print(f"Oops! The results exist at {p.cfg.OUTPUT_DIR} (so skip this job)")         # generate_classifier.sh:27-28
        return {}
    run = _open_job(p)                                        # process group, seed, bank, splits
    _build_trainer(p, run)                                    # weights, loaders, trainer
    _install_vocabulary(p, run)                               # generate | --classifiers | --bank and its edits
    return _close_job(p, run, _run_mode(p, run))                # the audit, the mode's pass and files; then reports, results, barrier


if __name__ == "__main__":
    main()
