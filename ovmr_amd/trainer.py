"""`MM_CLS_OP`: the evaluation / classifier-generation side of the reference's trainer class, on the HIP path.

Mirrors the names, call order and error behaviour of `MM_CLS_OP` (trainers/mm_classifier_one_prompt.py:367-493) and of
the `SimpleTrainer` methods it inherits for testing (Dassl.pytorch/dassl/engine/trainer.py:460-521), so a script written
against the reference

    trainer = build_trainer(cfg)                  # TRAINER_REGISTRY -> MM_CLS_OP(cfg)
    trainer.load_model(args.model_dir, epoch=args.load_epoch)
    trainer.test()

runs unchanged with `trainer = ovmr_amd.trainer.MM_CLS_OP(cfg, dm, clip_weights=...)`; the runner (ovmr_amd/cli.py) is such a
script.  Everything that needs autograd (forward_backward, the optimiser, save_model) is out of scope and
raises.

`dm` is anything with the four attributes the reference's DataManager (Dassl.pytorch/dassl/data/data_manager.py:116-170)
hands the trainer: `dataset.classnames`, `test_loader`, `val_loader` (may be None) and `eval_set_loader`
(`RandomClassSampler` batches: S consecutive rows per class).

`ZeroshotCLIP` / `ZeroshotCLIP2` (trainers/zsclip.py) are registered next to it with the same Dassl-facing methods; they need only
`dataset.classnames` and `test_loader`.  What Dassl's SimpleTrainer gives all three lives in `_EvalTrainer`; a trainer class states
`check_cfg`, `build_model`, `model_inference` and what differs from the shared passes (`explained`, `after_test`, `output_modes`).
"""
from __future__ import annotations

import collections
import os
import random
from collections import OrderedDict
from typing import Dict

import torch

from . import checkpoint, modules
from .evaluator import Classification
from .runtime import ALL_MODES

TRAINER_REGISTRY: Dict[str, type] = {}


class _EvalTrainer:
    """The evaluation side of Dassl's SimpleTrainer (trainer.py:321-521).  `reserve`: the engine's workspace reserve (images per
    batch, exemplar rows, classes); None = the trainer class's own default."""

    CLIP_FETCHED_BY = ""          # where the reference downloads the CLIP weights (the FileNotFoundError names it)
    NOT_TRAINED = ""              # the NotImplementedError of forward_backward / train / save_model

    def __init__(self, cfg, dm, clip_weights=None, tokenizer=None, device: str = "cuda:0", reserve=None, per_class_result=False,
                 compute_cmat=False, score_curves=None, score_range=None, exact_curves=False, exact_max_bytes=None):
        self.check_cfg(cfg)
        self.cfg, self.dm, self.device = cfg, dm, torch.device(device)
        self._clip_weights, self._tokenizer, self._reserve = clip_weights, tokenizer, reserve
        self._models: "OrderedDict[str, object]" = OrderedDict()
        self.test_loader = dm.test_loader
        self.val_loader = getattr(dm, "val_loader", None)
        self.eval_set_loader = getattr(dm, "eval_set_loader", None)      # data_manager.py:157-170
        self.num_classes = len(dm.dataset.classnames)
        self.epoch = 0
        self.output_dir = cfg.OUTPUT_DIR
        self.build_model()
        # per_class_result / compute_cmat: what the reference reads from TEST.PER_CLASS_RESULT / TEST.COMPUTE_CMAT (evaluator.py:38, 165)
        self._evaluator_args = dict(per_class=per_class_result, confusion=compute_cmat)
        # score_curves = BINS: every evaluator of the pass keeps the per-class score histograms over score_range (evaluator.Classification:
        # curves=, score_range=; None = its default (0, 1), the range of MM_CLS_OP's probabilities -- logits have no natural range)
        if score_range is not None and score_curves is None:
            raise ValueError("score_range= belongs to score_curves=BINS")
        if score_curves is not None:
            self._evaluator_args.update(curves=score_curves, **({} if score_range is None else {"score_range": tuple(score_range)}))
        # exact_curves: every evaluator of the pass keeps its outputs and derives the exact per-class AP / AUROC from them at the end
        # (evaluator.Classification: exact=, exact_max_bytes=; None = its default budget).  Any score will do: no range
        if exact_max_bytes is not None and not exact_curves:
            raise ValueError("exact_max_bytes= belongs to exact_curves=True")
        if exact_curves:
            self._evaluator_args.update(exact=True, **({} if exact_max_bytes is None else {"exact_max_bytes": int(exact_max_bytes)}))
        self.evaluator = self._new_evaluator()
        self.mode_evaluators = None                  # EVAL_MODE all: one Classification per mode of ALL_MODES, made by the first such test()

    def check_cfg(self, cfg):
        pass

    def _new_evaluator(self) -> Classification:
        return Classification(self.num_classes, list(self.dm.dataset.classnames), device=str(self.device), **self._evaluator_args)

    def build_model(self):
        raise NotImplementedError

    def load_clip(self) -> "modules.CLIPModel":
        """load_clip_to_cpu + clip_model.to(device) of the reference's build_model, from `clip_weights` (a path or a state dict)."""
        print(f"Loading CLIP (backbone: {self.cfg.MODEL.BACKBONE.NAME})")
        w = self._clip_weights
        if w is None:
            raise FileNotFoundError(f"{type(self).__name__} needs clip_weights= (an OpenAI CLIP .pt file or a state dict): "
                                    f"there is no download on this path ({self.CLIP_FETCHED_BY} fetches it in the reference)")
        sd = checkpoint.load_clip_state_dict(w) if isinstance(w, (str, os.PathLike)) else w
        return modules.build_model(sd, device=str(self.device))

    def register_model(self, name, model, optim=None, sched=None):
        self._models[name] = model

    def get_model_names(self, names=None):
        return list(self._models.keys()) if names is None else list(names)

    # trainer.py:515-521.  The copies are enqueued like the engine's and the evaluator's own (Engine._dev, Classification.process): a
    # batch that is already where it belongs costs nothing, and no batch makes the host wait for the stream
    def parse_batch_test(self, batch):
        return batch["img"].to(self.device, non_blocking=True), batch["label"].to(self.device, non_blocking=True)

    # trainer.py:461-493 -- the file handling lives in ovmr_amd.checkpoint (Dassl layout, "module." prefixes, dropped token buffers)
    def load_model(self, directory, epoch=None):
        if not directory:
            print("Note that load_model() is skipped as no pretrained model is given")
            return
        for name in self.get_model_names():
            state, saved_epoch, path = checkpoint.load_prompt_learner_checkpoint(directory, epoch, name)
            print(f'Loading weights to {name} from "{path}" (epoch = {saved_epoch})')
            self._models[name].load_state_dict(state, strict=False)

    # the three passes over input batches, on the models' shared methods (modules._TwoInFlight; a zero-shot model ignores the exemplar loader)
    def outputs(self, inputs):
        """model_inference for every input batch of the test pass, in order (the model keeps two batches in flight)."""
        return self.model.output_batches(inputs, eval_set_loader=self.eval_set_loader)

    def after_test(self):
        """What a trainer still owes once the last output has been counted."""

    def output_modes(self):
        """What `outputs` yields, known from the configuration before the first batch: ALL_MODES for [4, B, C] outputs (EVAL_MODE all: one
        evaluator per mode), None for [B, C] outputs (one evaluator).  A pass sharded over ranks decides its evaluators from this -- a rank
        without a batch has no output to look at."""
        return ALL_MODES if getattr(self.cfg, "EVAL_MODE", None) == "all" else None

    def _pass_group(self, data_loader):
        """The process group a pass over `data_loader` is sharded over: torch.distributed when the loader carries `batch_shard` with more
        than one rank, else None (every rank evaluates everything and nothing is reduced, as without a group).  A sharded loader without
        the matching group is refused here, before the first batch: the figures would be those of a part of the test set."""
        shard = getattr(data_loader, "batch_shard", None)
        if shard is None or shard[1] <= 1:
            return None
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError(f"the test loader holds the batches of rank {shard[0]} of {shard[1]} (batch_shard), but no torch.distributed "
                               "process group is initialised: the result would cover a part of the test set")
        if (dist.get_rank(), dist.get_world_size()) != tuple(shard):
            raise RuntimeError(f"the test loader holds the batches of rank {shard[0]} of {shard[1]} (batch_shard), this process is rank "
                               f"{dist.get_rank()} of {dist.get_world_size()}")
        return dist

    # trainer.py:460-482 (DATASET.REGION_AUG False)
    @torch.no_grad()
    def test(self, split=None):
        self.evaluator.reset()
        if split is None:
            split = getattr(getattr(self.cfg, "TEST", None), "SPLIT", "test")
        if split == "val" and self.val_loader is not None:
            data_loader = self.val_loader
        else:
            split = "test"
            data_loader = self.test_loader
        print(f"Evaluate on the *{split}* set")
        dist = self._pass_group(data_loader)
        labels = collections.deque()                 # an output is handed over after later batches have been fetched (two in flight)

        def inputs():
            for batch in data_loader:
                input, label = self.parse_batch_test(batch)
                labels.append(label)
                yield input

        topk = int(getattr(getattr(self.cfg, "TEST", None), "TOPK", 1))          # evaluator.process(mo, gt, topk), evaluator.py:50
        kw = {"topk": topk} if topk != 1 else {}
        per_mode = False
        if dist is not None:
            # sharded over ranks: the evaluators and their state exist before the loop, from the configuration, so that every rank calls the
            # same collectives with the same shapes whatever it received -- also a rank with no batch at all
            per_mode = self.output_modes() is not None
            if per_mode and self.mode_evaluators is None:
                self.mode_evaluators = [self._new_evaluator() for _ in ALL_MODES]
            evaluators = self.mode_evaluators if per_mode else [self.evaluator]
            for ev in evaluators:
                ev.reset()
                ev.begin(topk)
        for output in self.outputs(inputs()):
            label = labels.popleft()
            if dist is not None and (output.dim() == 3) != per_mode:
                raise RuntimeError(f"{type(self).__name__}.outputs yields {output.dim()}-dimensional outputs, output_modes() announced "
                                   f"{'[4, B, C]' if per_mode else '[B, C]'}: the ranks of a sharded pass agree on their evaluators up front")
            if output.dim() == 3:                    # [4, B, C] (EVAL_MODE all): plane p is mode ALL_MODES[p]'s output, counted by evaluator p
                if not per_mode:
                    per_mode = True
                    if self.mode_evaluators is None:
                        self.mode_evaluators = [self._new_evaluator() for _ in ALL_MODES]
                    for ev in self.mode_evaluators:
                        ev.reset()
                for ev, plane in zip(self.mode_evaluators, output):
                    ev.process(plane, label, **kw)
            else:
                self.evaluator.process(output, label, **kw)
        report = True
        if dist is not None:
            # each rank counted its own batches: after the sum every rank holds the job's counters (hence the same results); rank 0 reports
            Classification.all_reduce(evaluators, dist)
            report = dist.get_rank() == 0
        self.after_test()
        if not per_mode:
            self.results = self.evaluator.evaluate(self.output_dir or None, report=report)
            return list(self.results.values())[0]
        # one result block and one set of files (OUTPUT_DIR/<mode>/) per mode, every key prefixed "<mode>/"; then the table's four rows
        self.results = OrderedDict()
        for mode, ev in zip(ALL_MODES, self.mode_evaluators):
            if report:
                print(f"=> eval mode: {mode}")
            res = ev.evaluate(os.path.join(self.output_dir, mode) if self.output_dir else None, report=report)
            self.results.update((f"{mode}/{k}", v) for k, v in res.items())
        for mode in ALL_MODES if report else ():
            r = self.results
            print(f"=> {mode}: accuracy {r[mode + '/accuracy']:.1f}%, error {r[mode + '/error_rate']:.1f}%, macro_f1 {r[mode + '/macro_f1']:.1f}%")
        return list(self.results.values())[0]

    def ranked(self, inputs, k):
        """predict_topk for every input batch, in order: (values fp32 [B, k], indices int64 [B, k]) pairs."""
        return self.model.predict_topk_batches(inputs, k, eval_set_loader=self.eval_set_loader)

    @torch.no_grad()
    def predict(self, data_loader, k: int = 5):
        """Ranked prediction on unlabelled images (no counterpart in the reference): the k best classes of every image of `data_loader`
        (the loader protocol's batches; their labels are not read), best first, through the model's predict_topk_batches -- two batches
        in flight, ovmr_topk_rows on each output, ONE device-to-host copy at the end.  Returns (values fp32 [N, k], indices int64 [N, k])
        on the host, rows in loader order."""
        pairs = list(self.ranked((self.parse_batch_test(batch)[0] for batch in data_loader), k))
        self.after_test()
        if not pairs:
            return torch.zeros((0, k), dtype=torch.float32), torch.zeros((0, k), dtype=torch.int64)
        return torch.cat([v for v, _ in pairs]).cpu(), torch.cat([i for _, i in pairs]).cpu()

    def searched(self, inputs, m, within_top, base):
        """retrieve_batches over the input batches: the model's runtime.ColumnTopM."""
        return self.model.retrieve_batches(inputs, m, within_top, base, eval_set_loader=self.eval_set_loader)

    @torch.no_grad()
    def retrieve(self, data_loader, m: int = 32, within_top=None):
        """Search an unlabelled pool by class (no counterpart in the reference): the m best images of every class among the images of
        `data_loader` (the loader protocol's batches; their labels are not read), through the model's retrieve_batches -- two batches in
        flight, one ovmr_retrieve_update per output, the device-to-host copy at the end.  Returns (values fp32 [C, m], indices int64
        [C, m]) on the host: indices are positions in loader order, best first, equal scores to the lower position, -1 / -inf where a
        class has fewer than m images.  within_top = K: a class is searched only among the images that rank it within their K best
        scores (ties at the cut included).
        Under an initialised process group with a loader that carries `batch_shard` (and `batch_range`, `bs`: cli.FolderLoader,
        loader.PipelinedFolderLoader) every rank walks its own batches with the GLOBAL position of its first image as base, the states
        are all-gathered (int64 [C, m] each, shard.all_gather_retrieve_state) and merged on every rank: every rank returns the
        one-process result, bit for bit, because the state is a function of what was offered and not of who offered it."""
        dist = self._pass_group(data_loader)
        base = 0
        if dist is not None:
            base = int(data_loader.batch_range[0]) * int(data_loader.bs)
        top = self.searched((self.parse_batch_test(batch)[0] for batch in data_loader), m, within_top, base)
        if dist is not None:
            from .shard import all_gather_retrieve_state
            states = all_gather_retrieve_state(top.state, dist)
            for r in range(dist.get_world_size()):
                if r != dist.get_rank():
                    top.merge(states[r])
        self.after_test()
        values, indices = top.finish()
        return values.cpu(), indices.cpu()

    NO_EXEMPLARS = "nearest exemplars need a model that holds exemplar features (MM_CLS_OP only; a zero-shot trainer's classifier rows are text features)"

    def explained(self, inputs, k, n):
        """predict_explained for every input batch, in order: (values, indices, similarities, rows) per batch."""
        raise ValueError(f"--trainer {self.cfg.TRAINER.NAME}: {self.NO_EXEMPLARS}")

    @torch.no_grad()
    def predict_explained(self, data_loader, k: int = 5, n: int = 3):
        """predict() with the n nearest exemplars of every (image, predicted class): (values fp32 [N, k], indices int64 [N, k],
        similarities fp32 [N, k, n], rows int64 [N, k, n]) on the host, rows in loader order -- the first two are predict()'s."""
        outs = list(self.explained((self.parse_batch_test(batch)[0] for batch in data_loader), k, n))
        self.after_test()
        if not outs:
            return (torch.zeros((0, k), dtype=torch.float32), torch.zeros((0, k), dtype=torch.int64),
                    torch.zeros((0, k, n), dtype=torch.float32), torch.zeros((0, k, n), dtype=torch.int64))
        return tuple(torch.cat([o[i] for o in outs]).cpu() for i in range(4))

    def forward_backward(self, batch):
        raise NotImplementedError(self.NOT_TRAINED)

    train = save_model = forward_backward


class MM_CLS_OP(_EvalTrainer):
    """`prompt_learner_state`: the prompt learner's weights, already resolved by the caller; CustomCLIP then refuses an incomplete
    set (a later load_model can not: PromptLearner.load_state_dict counts the keys it holds as present) and MODEL.INIT_WEIGHTS is
    not read here."""

    CLIP_FETCHED_BY = "clip/clip.py:29-70"
    NOT_TRAINED = "training (autograd through CustomCLIP.forward, :310-338) is out of scope of the HIP hot path"

    def __init__(self, cfg, dm, clip_weights=None, tokenizer=None, device: str = "cuda:0", reserve=None, prompt_learner_state=None,
                 per_class_result=False, compute_cmat=False, score_curves=None, score_range=None, exact_curves=False, exact_max_bytes=None):
        self._prompt_learner_state = prompt_learner_state
        super().__init__(cfg, dm, clip_weights, tokenizer, device, reserve, per_class_result, compute_cmat, score_curves, score_range,
                         exact_curves, exact_max_bytes)

    # :369-370
    def check_cfg(self, cfg):
        assert cfg.TRAINER.COCOOP.PREC in ["fp16", "fp32", "amp"]

    # :372-419 (inference-relevant part: CLIP weights -> CustomCLIP -> optional INIT_WEIGHTS -> register "prompt_learner")
    def build_model(self):
        cfg = self.cfg
        random.seed(cfg.SEED)
        clip_model = self.load_clip()
        if cfg.TRAINER.COCOOP.PREC != "fp16":
            # the reference calls clip_model.float() here (:380-382) and then fails inside forward_prompt, whose buffers are
            # fp16 (:216-225): only fp16 evaluation exists
            raise RuntimeError("the OVMR evaluation path is fp16-only (trainers/mm_classifier_one_prompt.py:216-225)")
        print("Building custom CLIP")
        self.model = modules.CustomCLIP(cfg, self.dm.dataset.classnames, clip_model, tokenizer=self._tokenizer,
                                        prompt_learner_state=self._prompt_learner_state, reserve=self._reserve)
        init = getattr(cfg.MODEL, "INIT_WEIGHTS", "")
        if init and self._prompt_learner_state is None:                       # load_pretrained_weights (:403-404)
            ckpt = checkpoint._torch_load(init)
            self.model.prompt_learner.load_state_dict(ckpt["state_dict"] if "state_dict" in ckpt else ckpt, strict=False)
        self.register_model("prompt_learner", self.model.prompt_learner)     # :410

    # :454-459
    def parse_batch_train(self, batch):
        return self.parse_batch_test(batch)

    # trainer.py:504-508
    def model_inference(self, input, scale_no=0, label=None):
        if self.eval_set_loader is not None:
            return self.model(input, eval_set_loader=self.eval_set_loader, scale_no=scale_no, label=label)
        return self.model(input, label=label)

    def explained(self, inputs, k, n):
        return (self.model.predict_explained(image, k, n, eval_set_loader=self.eval_set_loader) for image in inputs)

    def audit_bank(self, k=5, classes=None, dup_threshold=0.995, batch=1024):
        """CustomCLIP.audit_bank on the trainer's model (generated in this run, or installed by load_bank)."""
        return self.model.audit_bank(k, classes, dup_threshold, batch)

    def after_test(self):
        self.model.wait_files()                      # mm_classifiers.pt / visual_tokens.pt were written while the test set ran


TRAINER_REGISTRY["MM_CLS_OP"] = MM_CLS_OP


class ZeroshotCLIP(_EvalTrainer):
    """trainers/zsclip.py:32-60 (BASELINE configuration 1).  `dm` needs `dataset.classnames` and `test_loader` (`val_loader` optional);
    cfg.DATASET.NAME picks the template (ovmr_amd.templates).  Nothing is trained and nothing is registered, so load_model has nothing
    to load."""

    MODULE = modules.ZeroshotCLIP
    CLIP_FETCHED_BY = "trainers/coop.py load_clip_to_cpu"
    NOT_TRAINED = "the zero-shot trainers have nothing to train"

    def check_cfg(self, cfg):
        from . import templates
        templates.check_dataset(cfg.DATASET.NAME)                           # (the reference's CUSTOM_TEMPLATES lookup, :42 / :83)

    def build_model(self):
        cfg = self.cfg
        classnames = self.dm.dataset.classnames
        self.clip_model = self.load_clip()                                   # :38
        reserve = self._reserve
        if reserve is None:
            batch = getattr(getattr(cfg.DATALOADER, "TEST", None), "BATCH_SIZE", 256)
            reserve = (batch, 256, max(1024, len(classnames)))
        self.model = self.MODULE.from_classnames(self.clip_model, classnames, cfg.DATASET.NAME, self._tokenizer, reserve=reserve)
        self.text_features = self.model.text_features

    def model_inference(self, image):
        return self.model.model_inference(image)                             # :55-60

    def output_modes(self):
        return None                                  # (the zero-shot trainers ignore EVAL_MODE: [B, C] logits whatever it says)


class ZeroshotCLIP2(ZeroshotCLIP):
    """trainers/zsclip.py:63-99: prompt ensembling over IMAGENET_TEMPLATES_SELECT (+ the dataset's template off ImageNet)."""

    MODULE = modules.ZeroshotCLIP2


TRAINER_REGISTRY["ZeroshotCLIP"] = ZeroshotCLIP
TRAINER_REGISTRY["ZeroshotCLIP2"] = ZeroshotCLIP2


class LinearProbe(_EvalTrainer):
    """lpclip/linear_probe.py on the device: a logistic regression on the image features of the exemplars `dm.eval_set_loader` yields
    (or of a reference bank: fit_probe(features=, shots=)), evaluated by the shared test pass.  probe_c: the strength C of a fixed fit.
    Nothing is registered, so load_model has nothing to load.  Under torch.distributed every rank fits the same probe from the same
    exemplars -- the kernels are deterministic, so the ranks' probes are bit-equal -- and only the test pass is sharded."""

    CLIP_FETCHED_BY = "lpclip/feat_extractor.py"
    NOT_TRAINED = "the linear probe is fitted by fit_probe (L-BFGS on the device), not by Dassl's training loop"

    def __init__(self, cfg, dm, clip_weights=None, tokenizer=None, device: str = "cuda:0", reserve=None, probe_c: float = 1.0, **kw):
        self.probe_c = float(probe_c)
        super().__init__(cfg, dm, clip_weights, tokenizer, device, reserve, **kw)

    def build_model(self):
        cfg = self.cfg
        classnames = self.dm.dataset.classnames
        self.clip_model = self.load_clip()
        reserve = self._reserve
        if reserve is None:
            batch = getattr(getattr(cfg.DATALOADER, "TEST", None), "BATCH_SIZE", 256)
            reserve = (batch, 256, max(1024, len(classnames)))
        self.model = modules.LinearProbe(self.clip_model, classnames, reserve=reserve)

    def _fitted(self, state, search=None):
        """A fitted state becomes the model's probe, OUTPUT_DIR/linear_probe.pt and one line of the result block."""
        from . import probe
        state.search = search
        self.model.install(state)
        self.probe_state = state
        if self.output_dir and self._is_rank0():
            state.write(os.path.join(self.output_dir, probe.PROBE_FILE))
        self.probe_line = (f"=> linear probe: C {state.c:g} iterations {state.n_iter} converged {state.converged} "
                           f"train loss {getattr(state, 'loss', float('nan')):.6f}")
        return state

    @staticmethod
    def _is_rank0() -> bool:
        import torch.distributed as dist
        return not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0

    def _exemplars(self, features, shots):
        if features is not None:
            return features, shots
        if self.eval_set_loader is None:
            raise ValueError("LinearProbe.fit_probe needs exemplars: dm.eval_set_loader, or features= and shots= of a reference bank")
        return self.model.exemplar_features(self.eval_set_loader)

    @torch.no_grad()
    def fit_probe(self, c=None, features=None, shots=None):
        """Fits at strength c (default: probe_c) on the exemplar loader's images, or on features fp16 [R, D] / shots [C] packed class
        after class (a reference bank's fields).  -> probe.LinearProbeState, installed and written."""
        features, shots = self._exemplars(features, shots)
        return self._fitted(self.model.fit_features(features, shots, self.probe_c if c is None else float(c), install=False))

    @torch.no_grad()
    def search_probe(self, val_features, val_labels, steps: int = 8, features=None, shots=None):
        """The reference's search of C (probe.search_c) against validation features fp16 / fp32 [V, D] and labels int64 [V], both kept on
        the device: every candidate is fitted on the exemplars and scored by its top-1 accuracy there (the library's tie rule)."""
        from . import probe, runtime
        features, shots = self._exemplars(features, shots)
        vx = val_features.to(self.device).float().contiguous()
        vy = val_labels.to(self.device).reshape(-1, 1)

        def accuracy_at(state):
            scores = runtime.probe_logits(vx, state.W.to(self.device), state.b.to(self.device))
            return float((runtime.topk_rows(scores, 1)[1].long() == vy).double().mean())
        c, state, trace = probe.search_c(lambda c: self.model.fit_features(features, shots, c, install=False), accuracy_at, steps)
        return self._fitted(state, trace)

    def install_probe(self, path: str):
        """Installs a written linear_probe.pt; nothing is fitted."""
        from . import probe
        state = probe.LinearProbeState.read(path)
        if state.classnames != [str(n) for n in self.dm.dataset.classnames]:
            raise ValueError(f'"{path}": classnames are not this run\'s {self.num_classes} classes')
        self.model.install(state)
        self.probe_state = state
        return state

    def outputs(self, inputs):
        if self.model.W is None:
            self.fit_probe()
        return super().outputs(inputs)

    def ranked(self, inputs, k):
        if self.model.W is None:
            self.fit_probe()
        return super().ranked(inputs, k)

    def searched(self, inputs, m, within_top, base):
        if self.model.W is None:
            self.fit_probe()
        return super().searched(inputs, m, within_top, base)

    def after_test(self):
        if getattr(self, "probe_line", None) and self._is_rank0():
            print(self.probe_line)

    def model_inference(self, image):
        return self.model.model_inference(image)

    def output_modes(self):
        return None


TRAINER_REGISTRY["LinearProbe"] = LinearProbe


def build_trainer(cfg, dm, **kw):
    """dassl.engine.build_trainer: look the class up by cfg.TRAINER.NAME."""
    name = getattr(cfg.TRAINER, "NAME", "MM_CLS_OP")
    if name not in TRAINER_REGISTRY:
        raise ValueError(f"unknown trainer {name!r}; on the hot path: {sorted(TRAINER_REGISTRY)}")
    return TRAINER_REGISTRY[name](cfg, dm, **kw)
