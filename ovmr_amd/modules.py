"""Host-side mirror of the reference's module API for the OVMR hot path (orchestration only).

Same names, argument meaning, return types and file formats as
trainers/mm_classifier_one_prompt.py (`TextEncoder` :63-91, `PromptLearner` :94-176,
`CustomCLIP` :179-364) and clip/model.py:`build_model` (:899-936); every piece of arithmetic is
a call into libovmr_hip.so through ovmr_amd.runtime.Engine.  Nothing here computes on the CPU and
nothing falls back when the HIP library or the GPU is missing.

Differences a reference user will notice (all documented in DESIGN.md):
  * `clip_model` is a `CLIPModel` (weights + architecture), not an nn.Module;
  * class names are tokenised with the CLIP merge table named by OVMR_BPE_PATH (or ./clip/bpe_simple_vocab_16e6.txt.gz);
    `tokenizer=` (an object with the reference SimpleTokenizer's `encode(str) -> list[int]`) or already tokenised
    prompts (LongTensor [C, 77]) in place of `classnames` are accepted too;
  * the training branch of CustomCLIP.forward (:310-338) is out of scope and raises;
  * with torch.distributed initialised, forward_prompt shards the eval-set batches over ranks,
    all-gathers the classifier rows (RCCL) and all-reduces the F1 counters.
"""
from __future__ import annotations

import os
import os.path as osp
from types import SimpleNamespace
from typing import Dict, Iterable, List, Optional, Sequence, Union

import numpy as np
import torch

from . import synth
from .runtime import Engine
from .synth import ModelSpec, SOT_ID, EOT_ID


# ----------------------------------------------------------------------------- torch.save of host copies, tagged as the device tensors they mirror
_LOCATION_OVERRIDE: Dict[int, int] = {}          # storage data_ptr -> index of the device its values came from


def _override_tagger(storage):
    """torch.serialization location tagger (register_package): storages listed in _LOCATION_OVERRIDE are written with that location --
    "cuda:0" for the page-locked host copy of a device tensor, so that the archive equals a torch.save of the device tensor itself and
    reloads onto the device as the reference's files do (trainers/mm_classifier_one_prompt.py:276-291 saves CUDA tensors)."""
    if not _LOCATION_OVERRIDE:
        return None
    idx = _LOCATION_OVERRIDE.get(storage.data_ptr())
    # a NEW string per storage, as torch's own tagger builds it: the pickler memoises by object identity, and one shared tag object would
    # be written once and referenced afterwards -- other bytes than a torch.save of the device tensors
    return None if idx is None else "cuda:" + str(idx)


torch.serialization.register_package(1, _override_tagger, lambda storage, location: None)


class _saved_as_on_device:
    def __init__(self, tensors, device_index: int):
        self.keys, self.tag = [t.untyped_storage().data_ptr() for t in tensors], int(device_index)

    def __enter__(self):
        for k in self.keys:
            _LOCATION_OVERRIDE[k] = self.tag

    def __exit__(self, *exc):
        for k in self.keys:
            _LOCATION_OVERRIDE.pop(k, None)


# ----------------------------------------------------------------------------- CLIP weights
def infer_spec(state_dict: Dict[str, torch.Tensor], name: str = "from_state_dict") -> ModelSpec:
    """Architecture inference of build_model(), clip/model.py:899-928 (ViT branch only)."""
    if "visual.proj" not in state_dict:
        raise ValueError("only ViT CLIP models are on the hot path (ModifiedResNet is out of scope)")
    vision_width = state_dict["visual.conv1.weight"].shape[0]
    vision_layers = len([k for k in state_dict if k.startswith("visual.") and k.endswith(".attn.in_proj_weight")])
    patch = state_dict["visual.conv1.weight"].shape[-1]
    grid = round((state_dict["visual.positional_embedding"].shape[0] - 1) ** 0.5)
    embed_dim = state_dict["text_projection"].shape[1]
    context_length = state_dict["positional_embedding"].shape[0]
    vocab_size = state_dict["token_embedding.weight"].shape[0]
    width = state_dict["ln_final.weight"].shape[0]
    layers = len(set(k.split(".")[2] for k in state_dict if k.startswith("transformer.resblocks")))
    return ModelSpec(name, embed_dim, patch * grid, vision_layers, vision_width, patch, context_length,
                     vocab_size, width, width // 64, layers)


class CLIPModel:
    """Stands where the reference passes `clip_model`: weights in the reference state-dict layout."""

    def __init__(self, state_dict: Dict[str, "torch.Tensor"], spec: Optional[ModelSpec] = None,
                 device: str = "cuda:0"):
        self._sd = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in state_dict.items()}
        self.spec = spec or infer_spec(self._sd)
        self.device = torch.device(device)
        self.dtype = torch.float16                      # convert_weights(), clip/model.py:934
        self.visual = SimpleNamespace(output_dim=self.spec.embed_dim, input_resolution=self.spec.image_resolution)
        self.logit_scale = self._sd["logit_scale"].float()
        self.context_length = self.spec.context_length
        self.vocab_size = self.spec.vocab_size
        self._engines: Dict[int, Engine] = {}

    def state_dict(self):
        return self._sd

    def engine(self, n_ctx: int) -> Engine:
        if n_ctx not in self._engines:
            e = Engine(self.spec, n_ctx, str(self.device))
            e.load_state_dict(self._sd)
            self._engines[n_ctx] = e
        return self._engines[n_ctx]

    # CLIP.encode_image / encode_text (clip/model.py:814-833), used by the zero-shot baseline
    def encode_image(self, image, n_ctx: int = 2):
        return _ensure_final(self.engine(n_ctx)).encode_image(image, normalize=False)

    def encode_text(self, text, n_ctx: int = 2):
        return _ensure_final(self.engine(n_ctx)).encode_text_ids(text, normalize=0)


def build_model(state_dict: Dict[str, "torch.Tensor"], device: str = "cuda:0") -> CLIPModel:
    """clip/model.py:899-936."""
    return CLIPModel(state_dict, None, device)


def _ensure_final(e: Engine) -> Engine:
    if not e.finalized:
        if not hasattr(e, "_pl_loaded"):
            raise RuntimeError("prompt-learner weights have not been loaded into the engine yet")
        e.finalize(*getattr(e, "_reserve", (256, 256, 1024)))
    return e


def make_cfg(n_ctx: int = 2, num_shots: int = 16, eval_mode: str = "fusion", eval_tau: float = 10.0,
             output_dir: str = "output_ovmr/generated_classifiers", backbone: str = "ViT-B/16",
             test_batch_size: int = 256, size: int = 224) -> SimpleNamespace:
    """The cfg keys the hot path reads, as a plain namespace tree (no yacs)."""
    return SimpleNamespace(
        TRAINER=SimpleNamespace(COCOOP=SimpleNamespace(N_CTX=n_ctx, PREC="fp16")),
        INPUT=SimpleNamespace(SIZE=(size, size)),
        DATALOADER=SimpleNamespace(TRAIN_X=SimpleNamespace(BATCH_SIZE=1536, N_INS=8), K_TRANSFORMS=1,
                                   TEST=SimpleNamespace(BATCH_SIZE=test_batch_size)),
        DATASET=SimpleNamespace(NUM_SHOTS=num_shots),
        MODEL=SimpleNamespace(BACKBONE=SimpleNamespace(NAME=backbone), INIT_WEIGHTS=""),
        EVAL_MODE=eval_mode, EVAL_TAU=eval_tau, OUTPUT_DIR=output_dir, SEED=1)


_DEFAULT_TOKENIZER = {}


def default_tokenizer():
    """BPETokenizer on the CLIP merge table named by OVMR_BPE_PATH, or found at ./clip/bpe_simple_vocab_16e6.txt.gz (the
    working directory of a reference checkout).  FileNotFoundError when neither exists: the table is not shipped here."""
    from .tokenizer import BPETokenizer
    path = os.environ.get("OVMR_BPE_PATH") or osp.join("clip", "bpe_simple_vocab_16e6.txt.gz")
    if path not in _DEFAULT_TOKENIZER:
        if not osp.exists(path):
            raise FileNotFoundError("class names need the CLIP BPE merge table: set OVMR_BPE_PATH to bpe_simple_vocab_16e6.txt.gz "
                                    "(it is in every CLIP checkout), pass tokenizer=, or pass tokenised prompts [C,77] instead of names")
        _DEFAULT_TOKENIZER[path] = BPETokenizer(path)
    return _DEFAULT_TOKENIZER[path]


def tokenize(texts: Sequence[str], tokenizer, context_length: int = 77) -> torch.Tensor:
    """clip.tokenize (clip/clip.py:187-223) on top of a caller-supplied BPE `tokenizer.encode`."""
    out = torch.zeros(len(texts), context_length, dtype=torch.long)
    for i, t in enumerate(texts):
        ids = [SOT_ID] + list(tokenizer.encode(t)) + [EOT_ID]
        if len(ids) > context_length:
            raise RuntimeError(f"Input {t} is too long for context length {context_length}")
        out[i, :len(ids)] = torch.tensor(ids)
    return out


# ----------------------------------------------------------------------------- TextEncoder
class TextEncoder:
    """trainers/mm_classifier_one_prompt.py:63-91."""

    def __init__(self, clip_model: CLIPModel, n_ctx: int = 2):
        self.clip_model = clip_model
        self.n_ctx = n_ctx
        self.dtype = torch.float16                     # hard-coded in the reference (:70)

    def forward(self, prompts: torch.Tensor, eos_index: torch.Tensor, seq_len: Optional[int] = None) -> torch.Tensor:
        e = _ensure_final(self.clip_model.engine(self.n_ctx))
        return e.encode_text_embedded(prompts, eos_index, seq_len, normalize=0)

    __call__ = forward


# ----------------------------------------------------------------------------- PromptLearner
class PromptLearner:
    """trainers/mm_classifier_one_prompt.py:94-176 (inference path)."""

    def __init__(self, cfg, classnames, clip_model: CLIPModel, tokenizer=None,
                 state_dict: Optional[Dict[str, "torch.Tensor"]] = None, compute_zero_shot: bool = True,
                 reserve=(256, 256, 1024)):
        self.cfg = cfg
        self.n_ctx = n_ctx = cfg.TRAINER.COCOOP.N_CTX
        self.dtype = torch.float16
        spec = clip_model.spec
        self.clip_model = clip_model
        self.engine = e = clip_model.engine(n_ctx)
        e._reserve = reserve
        dev = e.device
        self.tokenizer = tokenizer
        self.install_vocabulary(classnames, embed=False)
        vt = torch.from_numpy(synth.template_token_ids(spec.context_length))        # "a ." (:114-115)

        # trainable state: cls_token + aggregator; random CLIP-style init when absent (:145-154)
        if state_dict is None:
            state_dict = {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, n_ctx, cfg.SEED).items()}
        self._state: Dict[str, torch.Tensor] = {}
        self.load_state_dict(state_dict, strict=True)
        _ensure_final(e)

        self._embed_vocabulary()                                                    # :129,131
        self.visual_prompt_temp = e.embed_tokens(vt.to(dev))                        # :130
        # :118-126.  The reference skips this for num_class >= 5000 and then fails at :265 ("limits the
        # build must lift"); here such vocabularies get their text rows batch by batch inside forward_prompt instead.
        self.zero_shot_classifier = None
        if compute_zero_shot and self.num_class < 5000:
            self.zero_shot_classifier = self.encode_zero_shot(self.tokenized_prompts)

    def tokenize_names(self, classnames: Sequence[str]) -> torch.Tensor:
        """The token rows [n, context_length] of "a <name>." for every class name (:109-116), on the host."""
        if self.tokenizer is None:
            # the reference's module-level `_tokenizer = _Tokenizer()` (:26) reads the merge table that sits next to
            # clip/simple_tokenizer.py; here it comes from OVMR_BPE_PATH or ./clip/bpe_simple_vocab_16e6.txt.gz
            self.tokenizer = default_tokenizer()
        names = [n.replace("_", " ") for n in classnames]                           # :109
        return tokenize(["a " + n + "." for n in names], self.tokenizer, self.clip_model.spec.context_length)   # :113,116

    def install_vocabulary(self, classnames, embed: bool = True, prompt_tokens: Optional[torch.Tensor] = None):
        """Installs a vocabulary -- class names, or their token rows [C, context_length] -- and derives every table that depends on it, HERE
        and nowhere else: num_class, name_lens, tokenized_prompts, eos_index, max_eos (and, with `embed`, prompt_tokens: taken from
        `prompt_tokens` when the caller already holds the embedded rows, embedded otherwise).  __init__ and the vocabulary edits of
        CustomCLIP (load_bank, add / replace / remove_classes) go through it.  name_lens is the EOT position minus the three tokens of
        the template "a <name>." (SOT, "a", ".") for token rows, len(tokenizer.encode(name)) (:110) for names."""
        dev = self.engine.device
        if isinstance(classnames, (torch.Tensor, np.ndarray)):
            tokenized = torch.as_tensor(classnames).long().cpu()
            self.name_lens = (tokenized.argmax(-1) - 3).tolist()
        else:
            tokenized = self.tokenize_names(classnames)
            self.name_lens = [len(self.tokenizer.encode(n.replace("_", " "))) for n in classnames]   # :110
        self._tokenized_host = tokenized
        self._eos_host = tokenized.argmax(-1)
        self.num_class = self.n_cls = tokenized.shape[0]
        self.max_eos = int(self._eos_host.max())
        self.tokenized_prompts = tokenized.to(dev)
        self.eos_index = self._eos_host.to(dev)
        if embed:
            self._embed_vocabulary(prompt_tokens)

    def _embed_vocabulary(self, prompt_tokens: Optional[torch.Tensor] = None):
        self.prompt_tokens = self.engine.embed_tokens(self.tokenized_prompts) if prompt_tokens is None else prompt_tokens   # :129,131

    def encode_zero_shot(self, tokenized: torch.Tensor) -> torch.Tensor:
        """:118-126 -- per class encode_text of its prompt, mean over the single prompt, F.normalize."""
        return self.engine.encode_text_ids(tokenized, seq_len=self.max_eos + 1, normalize=1)

    # nn.Module-like state API
    def state_dict(self) -> Dict[str, torch.Tensor]:
        return dict(self._state)

    def load_state_dict(self, state_dict, strict: bool = False):
        expected = set(synth.prompt_learner_keys(self.clip_model.spec))
        sd = {k: v for k, v in state_dict.items() if k not in ("token_prefix", "token_suffix")}     # :482-487
        unknown = set(sd) - expected
        missing = expected - set(sd) - set(self._state)
        if strict and (unknown or missing):
            raise RuntimeError(f"PromptLearner.load_state_dict: missing {sorted(missing)}, unexpected {sorted(unknown)}")
        for k, v in sd.items():
            if k in expected:
                t = (torch.from_numpy(v) if isinstance(v, np.ndarray) else v).detach().float()
                self._state[k] = t
                self.engine.set_weight("prompt_learner." + k, t)
        self.engine._pl_loaded = True
        if not missing:
            self.engine.finalize(*self.engine._reserve)
        return SimpleNamespace(missing_keys=sorted(missing), unexpected_keys=sorted(unknown))

    @property
    def cls_token(self):
        return self._state["cls_token"]

    def eval(self):
        return self

    training = False

    def update_prompts(self, prompt_tokens, ins_tokens):
        """:156-157 (kept for API parity; forward uses the fused assemble kernel)."""
        return torch.cat([prompt_tokens[:, :2], ins_tokens.type(self.prompt_tokens.dtype),
                          prompt_tokens[:, 2:-self.n_ctx]], dim=1)

    def forward(self, exemplar_img_feats: torch.Tensor, label: torch.Tensor, ori_text_len: torch.Tensor, shots=None):
        """:159-176 -> (mm_prompts_list, mm_lens, v_prompts_list, v_lens, agg_img_token_).  shots (a host sequence, one count per class
        of `label`): the features are packed [R, D], class after class, and every class's tokens come from exactly its own shots[c]
        rows (Engine.generate_tokens_ragged: per class the reference's arithmetic at num_ins = shots[c]); prompts, lengths and tokens
        are returned as without it."""
        e = self.engine
        mm_lens = ori_text_len + self.n_ctx                                                     # :163
        v_lens = torch.ones_like(ori_text_len, dtype=torch.int32) + self.n_ctx                  # :165
        if shots is not None:
            tokens = e.generate_tokens_ragged(exemplar_img_feats, shots)
        else:
            tokens = e.generate_tokens(exemplar_img_feats)                                      # :167-169
        mm = e.assemble_prompts(self.prompt_tokens, label, tokens)                              # :171
        v = e.assemble_prompts(self.visual_prompt_temp, None, tokens)                           # :173
        return [mm], mm_lens, [v], v_lens, tokens

    __call__ = forward


# ----------------------------------------------------------------------------- two test batches in flight
class _TwoInFlight:
    """The model calls of an evaluation loop, software-pipelined over two handles / two streams (CustomCLIP.forward_batches,
    ZeroshotCLIP.inference_batches).  A user defines `engine`, `device`, `_forward_on(engine, image[, out])`, `_twin_state()` and the hook
    `_before_outputs(what, eval_set_loader=None, one_mode=None)`: what the model owes before its first output -> the number of classes."""

    OVERLAP_MAX_TILES = 1024      # two batches in flight while the narrowest GEMM grid of ONE batch (ceil(rows / 256) x width / 256
                                  # workgroups of 256 x 256) stays within 4 rounds of the 256 CUs; beyond that a batch's partial last round is
                                  # a small share and two batches only contend (profiles/r03u_two_stream_sweep.log: ViT-B/16 128 / 256 / 384
                                  # images +26 / +7 / +4 %, 512 -2 %; ViT-L/14@336px 64 images +8 %, 128 -1 %, 256 -2 %)

    @property
    def OVERLAP_MAX_BATCH(self) -> int:
        """Images per batch up to which forward_batches keeps two batches in flight (settable; default from OVERLAP_MAX_TILES:
        ViT-B/16 443 images, ViT-L/14@336px 113)."""
        if getattr(self, "_overlap_max_batch", None) is not None:
            return self._overlap_max_batch
        sp = self.engine.spec
        tokens = (sp.image_resolution // sp.vision_patch_size) ** 2 + 1
        row_tiles = self.OVERLAP_MAX_TILES // max(1, sp.vision_width // 256)
        return max(1, row_tiles * 256 // tokens)

    @OVERLAP_MAX_BATCH.setter
    def OVERLAP_MAX_BATCH(self, n: int):
        self._overlap_max_batch = int(n)

    IN_FLIGHT = 2                 # test batches in flight in forward_batches / inference_batches: one handle + stream each

    def _twin(self, slot: int = 1) -> Engine:
        """Handle number `slot` (1 ... IN_FLIGHT - 1; 0 is the engine itself): the same weights and options, its own workspace (sized for
        OVERLAP_MAX_BATCH images), used from its own stream.  Rebuilt when the first handle's weights have changed since."""
        e = self.engine
        twins = self.__dict__.setdefault("_twin_engines", {})
        t = twins.get(slot)
        if t is None or t._twin_of_version != e._weights_version:
            t = Engine(e.spec, e.n_ctx, str(e.device))
            t.load_state_dict(*self._twin_state())
            t._pl_loaded = True
            res = getattr(e, "_reserve", (256, 256, 1024))
            t._reserve = (min(res[0], self.OVERLAP_MAX_BATCH), res[1], res[2])
            t._twin_of_version = e._weights_version
            twins[slot] = t
            if slot == 1:
                self._twin_engine = t
        for k, v in e._options.items():
            if t._options.get(k) != v:
                t.set_option(k, v)
        return _ensure_final(t)

    @staticmethod
    def _topk(out, k: int):
        """(values fp32 [B, k], indices int64 [B, k]) of a [B, C] output: ovmr_topk_rows on the current stream, the library's total
        order (include/ovmr_hip.h: larger first, ties to the lower column, NaN largest)."""
        from . import runtime
        values, indices = runtime.topk_rows(out, k)
        return values, indices.long()

    @torch.no_grad()
    def output_batches(self, batches: Iterable, eval_set_loader=None, overlap: Optional[bool] = None, stable_inputs: bool = False):
        """CustomCLIP.forward_batches and ZeroshotCLIP.inference_batches under one name (their docstrings say the rest): the model's output
        for every image batch, in order, two in flight.  What the model owes before its first output is the first next()'s, not the call's."""
        self._before_outputs("output_batches", eval_set_loader)
        yield from self._run_batches(batches, overlap, stable_inputs)

    def predict_topk_batches(self, batches: Iterable, k: int, eval_set_loader=None, overlap: Optional[bool] = None, stable_inputs: bool = False):
        """predict_topk for every image batch, in order, over forward_batches / inference_batches (two batches in flight): one (values,
        indices) pair per batch.  (The zero-shot models accept eval_set_loader for CustomCLIP's signature and do not read it.)"""
        outs = self.output_batches(batches, eval_set_loader, overlap, stable_inputs)
        return (self._topk(out, k) for out in outs)

    @torch.no_grad()
    def retrieve_batches(self, batches, m: int, within_top: Optional[int] = None, base: int = 0, eval_set_loader=None,
                         overlap: Optional[bool] = None, stable_inputs: bool = False):
        """Search a pool by class (no counterpart in the reference's API): the m best images of every class over the image batches of
        `batches`, two batches in flight as in the test loop; each output is offered to a runtime.ColumnTopM on the current stream as it is
        handed over, row b of a batch being image `base` + (rows of the earlier batches) + b.  Returns the ColumnTopM: finish() gives
        (values fp32 [C, m], indices int64 [C, m]) on the device, best first, equal scores to the lower image index, index -1 / value -inf
        where a class has fewer than m images; its `state` merges with that of other ranks (disjoint images).
        within_top = K (1 <= K <= min(32, C)): each batch first runs ovmr_topk_rows(out, K) and its K-th value is the row's floor, so a
        class is searched only among the images that rank it within their K best scores.  Ties at the cut are INCLUDED: an image whose
        score for a class equals its own K-th best score is eligible for that class, also where topk_rows listed another column of the
        same score."""
        from . import runtime
        what = "retrieve_batches"
        C, outs = self._before_outputs(what, eval_set_loader, "a search by class"), self._run_batches(batches, overlap, stable_inputs)   # (owed in the call)
        m = runtime._want_int(what, "m", m, 1, runtime.MAX_PER_CLASS)
        if within_top is not None:
            within_top = runtime._want_int(what, "within_top", within_top, 1, min(32, C))
        base = runtime._want_int(what, "base", base, 0, runtime.MAX_POOL)
        top = runtime.ColumnTopM(C, m, self.device)
        for out in outs:
            floor = None
            if within_top is not None:
                floor = runtime.topk_rows(out, within_top)[0][:, within_top - 1].contiguous()
            top.update(out, base, floor)
            base += int(out.shape[0])
        return top

    def _run_batches(self, batches, overlap, stable_inputs):
        cur = torch.cuda.current_stream(self.device)

        def hand_over(p):
            out, ev = p
            cur.wait_event(ev)
            out.record_stream(cur)
            return out

        cap = min(self.OVERLAP_MAX_BATCH, getattr(self.engine, "_reserve", (256,))[0])    # what the twin's workspace holds
        try:
            yield from self._forward_batches(batches, overlap, stable_inputs, cap, cur, hand_over)
        finally:                                         # also when the caller abandons the loop: later work on the caller's stream
            for st in getattr(self, "_overlap_streams", ()):     # (another forward on the first handle) is ordered behind what is in flight
                cur.wait_stream(st)

    def _forward_batches(self, batches, overlap, stable_inputs, cap, cur, hand_over):
        import collections
        n = max(2, int(self.IN_FLIGHT))
        pending = collections.deque()                    # (output, event on its stream), oldest first: at most n - 1 while the next is enqueued
        k = 0
        for image in batches:
            self.engine.check_image(image)               # refused before it is copied, staged or given a stream
            image = self.engine._dev(image)
            use = overlap if overlap is not None else image.shape[0] <= cap
            if not use or image.shape[0] > cap:
                while pending:
                    yield hand_over(pending.popleft())
                yield self._forward_on(self.engine, image)
                continue
            if len(getattr(self, "_overlap_streams", ())) < n:
                self._overlap_streams = [torch.cuda.Stream(self.device) for _ in range(n)]
                self._overlap_staging = [None] * n
            slot = k % n
            eng = self.engine if slot == 0 else self._twin(slot)
            st = self._overlap_streams[slot]
            if not stable_inputs:                        # (the previous user of this staging buffer, batch k - n, was handed over already:
                buf = self._overlap_staging[slot]        #  the current stream is ordered behind it)
                if buf is None or buf.shape[1:] != image.shape[1:] or buf.shape[0] < image.shape[0] or buf.dtype != image.dtype:
                    buf = self._overlap_staging[slot] = torch.empty((cap,) + tuple(image.shape[1:]),
                                                                    dtype=image.dtype, device=self.device)
                staged = buf[:image.shape[0]]
                staged.copy_(image)
                image = staged
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                out = self._forward_on(eng, image)
                ev = torch.cuda.Event()
                ev.record(st)
            if stable_inputs:
                image.record_stream(st)
            pending.append((out, ev))
            if len(pending) >= n:
                yield hand_over(pending.popleft())
            k += 1
        while pending:
            yield hand_over(pending.popleft())


# ----------------------------------------------------------------------------- CustomCLIP
class _ImageEncoder:
    """clip_model.visual as CustomCLIP uses it: callable, with .output_dim (:184, :216)."""

    def __init__(self, engine: Engine):
        self.engine = engine
        self.output_dim = engine.spec.embed_dim

    def __call__(self, image):
        return self.engine.encode_image(image, normalize=False)


class _RaggedRows:
    """The exemplar rows of a generation in ragged mode: a batch that carries "shots" (a HOST int64 tensor, one count per class; the
    batch's rows are class after class, "label" per row as ever) gives every class exactly the images it has.  The reference has no
    such mode: it takes NUM_SHOTS rows of every class by position (trainers/mm_classifier_one_prompt.py:237-245).  Keeps the packed
    features and their per-row labels for the cross-validation (CustomCLIP.eval_feat4cls / eval_row_labels) and the vocabulary's
    n_label = shots (the loader's `.shots`, int32 [C], known on every rank from the item list)."""

    def __init__(self, model, loader, world: int):
        self.model, self.loader, self.world = model, loader, world
        self.rows, self.labels, self.counted, self.uniform_seen = [], [], [], False
        n = getattr(loader, "shots", None)            # (a uniform loader may call its one count `shots`: only a per-class array is meant)
        self.vocabulary_shots = n if isinstance(n, (torch.Tensor, np.ndarray)) and n.ndim == 1 else None

    def takes(self, batch, batch_idx: int) -> bool:
        if "shots" not in batch:
            if self.rows:
                raise RuntimeError(f"eval-set batch {batch_idx} carries no \"shots\" while earlier batches did: one mode per loader")
            self.uniform_seen = True
            return False
        m = self.model
        if self.uniform_seen:
            raise RuntimeError(f"eval-set batch {batch_idx} carries \"shots\" while earlier batches did not: one mode per loader")
        if m.aug_times > 1 or isinstance(batch["img"], (list, tuple)):
            raise NotImplementedError("ragged exemplar sets (batches with \"shots\") do not take DATALOADER.K_TRANSFORMS > 1")
        # (every rank sees every batch of a loader that is not presharded, so every rank raises HERE, before the first collective)
        if self.world > 1 and not bool(getattr(self.loader, "presharded", False)):
            raise RuntimeError("ragged exemplar sets with more than one rank need a presharded (class-sharded) eval-set loader: the "
                               "round-robin bound of the all-gather assumes TEST.BATCH_SIZE // NUM_SHOTS classes per batch")
        if self.world > 1 and self.vocabulary_shots is None:
            raise RuntimeError("ragged exemplar sets with more than one rank need the loader's `.shots` (int32 [C], the whole vocabulary)")
        return True

    def encode(self, batch):
        """-> (feats [R, D] fp16, the classes' labels [n_cls] on the device, shots as a host list)."""
        m, dev = self.model, self.model.device
        shots = batch["shots"]
        if not isinstance(shots, torch.Tensor) or shots.is_cuda:
            raise ValueError("a batch's \"shots\" is a HOST int64 tensor [n_cls]")
        shots = [int(n) for n in shots.tolist()]
        label = batch["label"]
        if sum(shots) != label.shape[0] or min(shots, default=1) < 1:
            raise ValueError(f"a batch's shots {shots} do not describe its {label.shape[0]} rows")
        first = torch.tensor([0] + shots[:-1], dtype=torch.long).cumsum(0)
        exemplar_label = label.to(dev, non_blocking=True)
        feats = m.engine.encode_image(batch["img"], normalize=True)
        self.rows.append(feats)
        self.labels.append(exemplar_label.to(torch.int32))
        exemplar_label = exemplar_label[first.to(dev)]
        self.counted.append((exemplar_label, torch.tensor(shots, dtype=torch.int32)))
        return feats, exemplar_label, shots

    def finish(self):
        m, dev = self.model, self.model.device
        if self.uniform_seen or (not self.rows and self.vocabulary_shots is None):
            return                                                                  # uniform mode: nothing of this class's is used
        C, D = len(m.tokenized_prompts), m.engine.spec.embed_dim
        m.eval_feat4cls = torch.cat(self.rows) if self.rows else torch.zeros((0, D), dtype=torch.float16, device=dev)
        m.eval_row_labels = torch.cat(self.labels) if self.labels else torch.zeros(0, dtype=torch.int32, device=dev)
        n_label = self.vocabulary_shots
        if n_label is not None:
            n_label = torch.as_tensor(n_label).to(device=dev, dtype=torch.int32)
            if n_label.shape != (C,):
                raise ValueError(f"the loader's shots describe {tuple(n_label.shape)} classes, the vocabulary has {C}")
        else:                                                                       # one process: the batches have said it all
            n_label = torch.zeros(C, dtype=torch.int32, device=dev)
            for labels, shots in self.counted:
                n_label[labels] = shots.to(dev)
        m._ragged_n_label = n_label


AGG_MAX_LEN_CEILING = 4096      # OVMR_AGG_MAX_LEN_CEILING (include/ovmr_hip.h): aggregator rows, n_ctx + shots, of one class


class CustomCLIP(_TwoInFlight):
    """trainers/mm_classifier_one_prompt.py:179-364 (evaluation / classifier-generation branch)."""

    def __init__(self, cfg, classnames, clip_model: CLIPModel, tokenizer=None,
                 prompt_learner_state: Optional[Dict] = None, reserve=None, distributed: Optional[bool] = None,
                 stream_text: bool = False):
        """distributed: None = shard over the default process group when it has more than one rank; True = take the sharded
        path whenever a process group is initialised (also with ONE rank: the collectives then run through the backend --
        RCCL for "nccl" -- on this rank's own rows, tests/test_hip_distributed.py); False = never.
        stream_text: the zero-shot text rows (:118-126) are not encoded up front by PromptLearner.__init__ but batch by batch inside
        forward_prompt, in the same text-tower pass as the batch's multimodal and vision prompts (what sharded ranks and
        vocabularies of >= 5000 classes always do); same rows, two tower passes fewer per loader batch."""
        self.cfg = cfg
        import torch.distributed as dist
        ready = dist.is_available() and dist.is_initialized()
        if distributed is None:
            distributed = ready and dist.get_world_size() > 1
        if distributed and not ready:
            raise RuntimeError("CustomCLIP(distributed=True) needs an initialised torch.distributed process group")
        self._dist = dist if distributed else None
        if reserve is None:
            reserve = (cfg.DATALOADER.TEST.BATCH_SIZE if hasattr(cfg.DATALOADER, "TEST") else 256, 256, 1024)
        # NUM_SHOTS is the per-class ceiling in both layouts (what --ragged-shots caps a class at).  Beyond 128 aggregator rows per class
        # the engine is told so BEFORE PromptLearner finalises it, so that its workspace holds such a class; up to 128 nothing is set and
        # the engine is what it always was.
        rows = cfg.TRAINER.COCOOP.N_CTX + int(cfg.DATASET.NUM_SHOTS)
        if rows > AGG_MAX_LEN_CEILING:
            raise ValueError(f"DATASET.NUM_SHOTS {cfg.DATASET.NUM_SHOTS}: n_ctx + NUM_SHOTS = {rows} aggregator rows per class, the engine "
                             f"takes at most {AGG_MAX_LEN_CEILING} (NUM_SHOTS <= {AGG_MAX_LEN_CEILING - cfg.TRAINER.COCOOP.N_CTX})")
        if rows > 128:
            e = clip_model.engine(cfg.TRAINER.COCOOP.N_CTX)
            if e._options.get("agg_max_len", 128) < rows:
                e.set_option("agg_max_len", rows)
        self.prompt_learner = PromptLearner(cfg, classnames, clip_model, tokenizer, prompt_learner_state,
                                            compute_zero_shot=self._dist is None and not stream_text, reserve=reserve)
        self._text_streamed = bool(stream_text) or self._dist is not None
        self.engine = self.prompt_learner.engine
        self.tokenized_prompts = self.prompt_learner.tokenized_prompts
        # the vocabulary's class names (None for a model built from token rows) and whether the exemplar features in eval_feat4cls are
        # those the classifier rows were generated from: what save_bank and the vocabulary edits need
        self.classnames = None if isinstance(classnames, (torch.Tensor, np.ndarray)) else list(classnames)
        self._has_features = False
        self._exemplar_paths = None
        self.image_encoder = _ImageEncoder(self.engine)
        self.text_encoder = TextEncoder(clip_model, self.prompt_learner.n_ctx)
        self.logit_scale = clip_model.logit_scale
        self.dtype = clip_model.dtype
        self.train_bs = cfg.DATALOADER.TRAIN_X.BATCH_SIZE
        self.num_ins = cfg.DATALOADER.TRAIN_X.N_INS
        self.test_num_ins = cfg.DATASET.NUM_SHOTS
        self.aug_times = cfg.DATALOADER.K_TRANSFORMS
        self.zero_shot_classifier = self.prompt_learner.zero_shot_classifier
        self.mm_classifier = None
        self.visual_classifer = None          # sic -- attribute name of the reference (:225)
        self.fusion_weight = None
        self.device = self.engine.device

    def eval(self):
        return self

    def _twin_state(self):
        return self.prompt_learner.clip_model.state_dict(), self.prompt_learner.state_dict()

    # :200-212
    def get_mm_v_feats(self, mm_prompts, mm_lens, v_prompts, v_lens, text_ids=None):
        """The reference runs the text encoder once on the multimodal prompts and once on the vision prompts (:202-203); here both
        prompt families -- and, with `text_ids` [Cb, 77], the zero-shot text prompts of the same classes (:118-126) -- share ONE pass
        of the tower (Engine.encode_text_groups: each family keeps its own truncated length).  Returns (mm, v) or (mm, v, text)."""
        pl = self.prompt_learner
        n_ctx = pl.n_ctx
        assert len(mm_prompts) == 1 and len(v_prompts) == 1
        # normalize=2: x/x.norm() (:204), mean over the single list element, F.normalize (:210)
        groups = [dict(prompts=mm_prompts[0], index=mm_lens, seq_len=pl.max_eos + n_ctx + 1, normalize=2),
                  dict(prompts=v_prompts[0], index=v_lens, seq_len=2 + n_ctx, normalize=2)]
        if text_ids is not None:
            groups.append(dict(ids=text_ids, seq_len=pl.max_eos + 1, normalize=1))
        return tuple(self.engine.encode_text_groups(groups))

    @staticmethod
    def _batch_images(batch, device):
        image = batch["img"]
        if isinstance(image, (list, tuple)):                                     # K_TRANSFORMS > 1 (:229-234)
            image = torch.cat([im.to(device).unsqueeze(1) for im in image], dim=1).flatten(0, 1)
        return image

    def _reset_generation_state(self):
        """The buffers forward_prompt fills (:216-225): classifier rows, visual tokens, exemplar features, the per-class
        initialised flags, and the text rows when they are produced batch by batch."""
        e, pl, dev = self.engine, self.prompt_learner, self.device
        C, S, D, n_ctx = len(self.tokenized_prompts), self.test_num_ins, e.spec.embed_dim, pl.n_ctx
        f16 = dict(dtype=torch.float16, device=dev)
        self.mm_classifier = torch.zeros((C, D), **f16)
        self.visual_classifer = torch.zeros((C, D), **f16)
        self.inference_text_initialized = torch.zeros(C, dtype=torch.int32, device=dev)
        self.visual_tokens = torch.ones((C, n_ctx, D), **f16)
        self.eval_feat4cls = torch.zeros((C, S, D), **f16)
        self.eval_row_labels = None           # ragged mode: eval_feat4cls is then the packed [R_local, D] rows, these their int32 labels
        self._ragged_n_label = None
        # text rows: precomputed by PromptLearner.__init__ (:118-126) for < 5000 classes in one process; otherwise
        # (large vocabularies, or class-sharded ranks) each exemplar batch encodes the prompts of its own classes
        streamed_text = pl.zero_shot_classifier is None or getattr(self, "_text_streamed", False)
        self._text_streamed = streamed_text
        self._text_rows = torch.zeros((C, D), **f16) if streamed_text else self.zero_shot_classifier

    def _exemplar_batches(self, eval_set_loader: Iterable, rank: int = 0, world: int = 1, gathered: bool = True, keep: Optional[list] = None):
        """The walk over an eval-set loader (:227-247): for every batch that belongs to `rank` of `world` its exemplar features are
        encoded and stored, and (feats, exemplar_label, shots) is handed out -- uniform mode: feats [num_cls, S, D], also written to
        eval_feat4cls[exemplar_label], shots None; ragged mode (_RaggedRows): feats the packed [R, D] rows, shots a host list.  The
        attributes of ragged mode are set when the walk ends.  gathered: the caller all-gathers per-batch blocks (forward_prompt).
        keep (a list; the vocabulary edits): the model's exemplar store is left alone -- every batch's (packed rows [n, D], class labels, shots
        as a host list) is appended to `keep` instead, and the edit puts the rows where they belong."""
        e, dev, S = self.engine, self.device, self.test_num_ins
        presharded = bool(getattr(eval_set_loader, "presharded", False))
        cpb = max(1, self.cfg.DATALOADER.TEST.BATCH_SIZE // S)
        ragged = _RaggedRows(self, eval_set_loader, world)
        for batch_idx, batch in enumerate(eval_set_loader):
            takes = ragged.takes(batch, batch_idx)                                  # every class uses exactly the images it has
            if not takes and gathered and world > 1 and not presharded and batch["label"].shape[0] // S > cpb:
                # every rank iterates over every batch of a round-robin loader, so every rank raises HERE, before any of them
                # has entered the all-gather whose block size assumes at most `cpb` classes per batch (shard.local_class_bound)
                raise RuntimeError(f"eval-set batch {batch_idx} holds {batch['label'].shape[0] // S} classes, more than "
                                   f"TEST.BATCH_SIZE // NUM_SHOTS = {cpb}")
            if not presharded and batch_idx % world != rank:
                continue
            if takes:
                out = ragged.encode(batch)
                if keep is not None:
                    keep.append(out)
                yield out
                continue
            image = self._batch_images(batch, dev)
            label = batch["label"].to(dev, non_blocking=True)
            num_cls = image.shape[0] // S                                            # :237
            exemplar_label = label.reshape(num_cls, S)[:, 0]                        # :240
            feats = e.encode_image(image, normalize=True).reshape(num_cls, S, -1)   # :243-245
            if keep is not None:
                keep.append((feats.flatten(0, 1), exemplar_label, [S] * num_cls))
            else:
                self.eval_feat4cls[exemplar_label] = feats                          # :247
            yield feats, exemplar_label, None
        if keep is None:
            ragged.finish()

    def _generate_local(self, eval_set_loader: Iterable, rank: int = 0, world: int = 1, keep: Optional[list] = None) -> torch.Tensor:
        """Hot loop A (:227-255) over the batches of `eval_set_loader` that belong to `rank` of `world`: exemplar features,
        visual tokens, multimodal / vision (and streamed text) classifier rows written at their class labels into the buffers
        of _reset_generation_state.  Returns the class labels this call produced, in order.  keep: see _exemplar_batches (the vocabulary
        edits run THIS loop on the edited classes' batches, with streamed text rows)."""
        pl = self.prompt_learner
        streamed_text, text_clf = self._text_streamed, self._text_rows
        local_labels = []
        for feats, exemplar_label, shots in self._exemplar_batches(eval_set_loader, rank, world, keep=keep):
            mm_p, mm_l, v_p, v_l, tokens = pl(feats, exemplar_label, pl.eos_index[exemplar_label], shots=shots)   # :248
            if streamed_text:                                                       # :249 + the batch's own zero-shot rows (:118-126), one tower pass
                mm, v, t = self.get_mm_v_feats(mm_p, mm_l, v_p, v_l, self.tokenized_prompts[exemplar_label])
                text_clf[exemplar_label] = t
            else:
                mm, v = self.get_mm_v_feats(mm_p, mm_l, v_p, v_l)                   # :249
            self.mm_classifier[exemplar_label] = mm                                 # :251
            self.visual_classifer[exemplar_label] = v                               # :252
            self.inference_text_initialized.index_fill_(0, exemplar_label, 1)       # :254 (`[...] = 1` copies the scalar from the host:
                                                                                    #  a synchronisation in the middle of the head)
            self.visual_tokens[exemplar_label] = tokens.half()                      # :255
            local_labels.append(exemplar_label)
        return torch.cat(local_labels) if local_labels else torch.zeros(0, dtype=torch.long, device=self.device)

    @torch.no_grad()
    def forward_prompt(self, eval_set_loader: Iterable, wait_files: bool = True):
        """:214-292.  Returns (mm_classifier, visual_classifer, fusion_weight) and writes
        mm_classifiers.pt / visual_tokens.pt into cfg.OUTPUT_DIR (rank 0 only when distributed).
        wait_files=False (what forward() passes when it generates the classifiers inside a test loop): the files are written behind the
        caller's back (_write_files) and are complete after wait_files(); the default returns with both files on disk, as the reference does."""
        e, pl, dev = self.engine, self.prompt_learner, self.device
        C, S, D, n_ctx = len(self.tokenized_prompts), self.test_num_ins, e.spec.embed_dim, pl.n_ctx
        dist = self._dist
        rank, world = (dist.get_rank(), dist.get_world_size()) if dist else (0, 1)
        f16 = dict(dtype=torch.float16, device=dev)
        self._reset_generation_state()
        presharded = bool(getattr(eval_set_loader, "presharded", False))
        cpb = max(1, self.cfg.DATALOADER.TEST.BATCH_SIZE // S)
        local = self._generate_local(eval_set_loader, rank, world)
        streamed_text, text_clf = self._text_streamed, self._text_rows

        if dist:
            # ONE all-gather (RCCL) of the packed classifier rows: [mm | v | text | tokens | label bits]; packing and
            # unpacking are one launch each (ovmr_pack_rows / ovmr_unpack_rows) -- a dozen indexing kernels before
            from .shard import all_gather_block, local_class_bound
            bound = local_class_bound(C, world, presharded, cpb)
            block = e.pack_rows(self.mm_classifier, self.visual_classifer, text_clf, self.visual_tokens, local, bound)
            gathered = all_gather_block(block, dist)
            self.mm_classifier, self.visual_classifer, text_clf, self.visual_tokens, seen = e.unpack_rows(gathered, C, D, n_ctx)
            self.inference_text_initialized = (seen[:C] == 1).to(torch.int32)       # every class from exactly one rank
            self._stray_rows = seen[C:]
        if streamed_text:
            self.zero_shot_classifier = self.prompt_learner.zero_shot_classifier = text_clf
        all_initialized = self.inference_text_initialized.bool().all()              # :259 -- read back below, behind the enqueued head:
        if dist:                                                                    # a host round trip here would idle the GPU in front of it
            all_initialized = all_initialized & (self._stray_rows == 0).all()
        self.fusion_weight = self._xval_fusion_weight(local, self.mm_classifier, self.visual_classifer,
                                                      self.zero_shot_classifier, float(self.cfg.EVAL_TAU))   # :261-274
        # rank 0's output files: conversions and device-to-host copies are enqueued HERE, behind the head and in front of the host's one
        # synchronisation (the host is still ahead of the GPU: nothing of it lands on the critical path); the writer starts once the check
        # has passed (the reference asserts before it saves, :259 / :276)
        writer = self._write_files() if rank == 0 and self.cfg.OUTPUT_DIR else None
        assert bool(all_initialized), "a class received no exemplar batch"          # :259
        self._has_features, self._exemplar_paths = world == 1, None                 # (a sharded rank holds its own classes' features only)
        if writer is not None:
            writer()
            if wait_files:
                self.wait_files()
        return self.mm_classifier, self.visual_classifer, self.fusion_weight

    # ------------------------------------------------------------------ the two output files, off the critical path
    FILE_WRITE_DELAY_S = 0.05     # the writer thread starts its work when wait_files() is called, or this long after the job (see _write_files)
    ASYNC_FILE_WRITE = True       # mm_classifiers.pt / visual_tokens.pt (:276-291) are written by a worker thread behind a side stream while the
                                  # caller goes on (the query loop of a test pass, the next rank's barrier); False: inline, as the reference does.
                                  # The files are the same bytes either way (tests/test_hip_parity.py::test_async_file_write_is_byte_identical).

    def _write_files(self):
        """:276-291.  The saved objects are what the reference saves -- fp32 classifiers and fp16 visual tokens tagged with the device they
        live on -- snapshotted on the caller's stream and copied to page-locked host buffers on a side stream; `torch.save` itself
        (pickling, the zip archive) runs in a worker thread once the copies have landed.  Returns the callable that starts the writer
        (forward_prompt calls it once its completeness check has passed).  wait_files() joins it: forward_prompt calls it before it writes again, MM_CLS_OP.test() / the CLI / bench.py's step
        before they report, and the interpreter joins the (non-daemon) thread at exit."""
        self.wait_files()
        out_dir = self.cfg.OUTPUT_DIR
        mm = {"text_classifier": self.zero_shot_classifier.float(),               # :276-285, all fp32
              "vision_classifier": self.visual_classifer.float(),
              "mm_classifier": self.mm_classifier.float(),
              "fusion_weight": self.fusion_weight.float()}

        def save(mm, vt):
            # each archive is written under its own name inside a scratch directory (torch.save names the archive's records after the
            # file: the bytes are those of a direct torch.save(obj, "<OUTPUT_DIR>/mm_classifiers.pt")) and moved into place whole, so a
            # reader never finds a half-written file under the final name
            os.makedirs(out_dir, exist_ok=True)
            scratch = osp.join(out_dir, f".partial.{os.getpid()}")
            os.makedirs(scratch, exist_ok=True)
            try:
                for obj, name in ((mm, "mm_classifiers.pt"), ({"visual_tokens": vt}, "visual_tokens.pt")):   # :276-291 (visual tokens fp16)
                    torch.save(obj, osp.join(scratch, name))
                    os.replace(osp.join(scratch, name), osp.join(out_dir, name))
            finally:
                import shutil
                shutil.rmtree(scratch, ignore_errors=True)

        if not self.ASYNC_FILE_WRITE:
            vt_now = self.visual_tokens.clone()              # (a copy: `visual_tokens` may be a view of a larger storage, which torch.save would write whole)
            return lambda: save(mm, vt_now)
        import threading
        vt = self.visual_tokens.clone()                      # (a later forward_prompt allocates new buffers, but a caller may write into this one)
        on_gpu = self.device.type == "cuda"                  # (the multi-process CPU tests drive this class with a host-side stand-in engine)
        if on_gpu:
            # The device-to-host copies are ENQUEUED here, by the caller's thread, on a side stream, into page-locked buffers kept from
            # job to job: an asynchronous copy returns at once.  (torch.save on the device tensors from the worker thread copies each
            # storage into pageable memory with a blocking hipMemcpy; while those ran -- 4 ms in all for 8 MB -- the caller's kernel
            # launches queued up behind the runtime, exactly when the GPU had just been drained by the generation's final check: a
            # sharded rank 0 lost 4 ms of its 86 to a write that was meant to cost it nothing.)  The worker thread waits for the copies'
            # event and pickles the HOST tensors; _saved_as_on_device makes torch.save tag their storages with the device the values
            # came from, so the archive is byte for byte the one torch.save of the device tensors writes.
            cur = torch.cuda.current_stream(self.device)
            ready = torch.cuda.Event()
            ready.record(cur)
            if not hasattr(self, "_file_stream"):
                self._file_stream, self._file_pinned = torch.cuda.Stream(self.device), {}
            side, copied = self._file_stream, torch.cuda.Event()
            host = {}
            with torch.cuda.stream(side):
                side.wait_event(ready)
                for name, t in list(mm.items()) + [("visual_tokens", vt)]:
                    buf = self._file_pinned.get(name)
                    if buf is None or buf.shape != t.shape or buf.dtype != t.dtype:
                        buf = self._file_pinned[name] = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
                    buf.copy_(t, non_blocking=True)
                    host[name] = buf
                copied.record(side)
            tag = self.device.index if self.device.index is not None else torch.cuda.current_device()

        go = threading.Event()

        def work():
            try:
                if not on_gpu:
                    return save(mm, vt)
                # The writer yields to the caller's launch loop: it starts its CPU work (waiting on the copies' event, pickling, 8 MB of
                # CRC and tmpfs writes) when the caller asks for the files (wait_files sets `go`) or FILE_WRITE_DELAY_S after the job, whichever
                # comes first.  Started at once, it cost a sharded rank 0 between 0.9 and 2.6 ms of its 86 (two passes on one box,
                # profiles/r06h_*): the first milliseconds after a generation are when the host enqueues the query batches, and a second busy
                # thread in the process slows exactly that; by the time anybody waits for the files the GPU has its work queued.
                go.wait(self.FILE_WRITE_DELAY_S)
                copied.synchronize()                         # (blocks this thread only; mm / vt stay referenced by this closure until then)
                with _saved_as_on_device(list(host.values()), tag):
                    save({k: host[k] for k in mm}, host["visual_tokens"])
            except BaseException as e:                       # noqa: BLE001 -- re-raised by wait_files() on the caller's thread
                self._file_error = e

        def start():
            self._file_error, self._file_go = None, go
            self._file_thread = threading.Thread(target=work, name="ovmr-classifier-files", daemon=False)
            self._file_thread.start()

        return start

    def wait_files(self):
        """Returns once the classifier files of the last forward_prompt are complete on disk (no-op when nothing is in flight); raises what
        the writer raised."""
        t = getattr(self, "_file_thread", None)
        if t is not None:
            self._file_go.set()
            t.join()
            self._file_thread = None
            err, self._file_error = getattr(self, "_file_error", None), None
            if err is not None:
                raise err

    def _xval_fusion_weight(self, local, mm_classifier, v_classifier, t_classifier, tau: float):
        """K18-K20: cross-validation argmax counts on the exemplars this rank encoded (`local` = their class labels,
        features in self.eval_feat4cls), all-reduced over ranks, then F1 and softmax(tau * F1).  Column order mm, v, t."""
        e, dev, dist = self.engine, self.device, self._dist
        C, S = len(self.tokenized_prompts), self.test_num_ins
        counts = torch.zeros((3, 2, C), dtype=torch.int32, device=dev)
        ragged = getattr(self, "eval_row_labels", None) is not None
        if ragged or local.numel():
            if ragged:                                                              # the packed rows as they are, a label per row
                rows, row_labels = self.eval_feat4cls, self.eval_row_labels
            else:
                rows = self.eval_feat4cls[local].flatten(0, 1)
                row_labels = local.to(torch.int32).unsqueeze(1).expand(-1, S).reshape(-1)   # :261 (repeat_interleave: five launches for the same rows)
            for m, clf in enumerate((mm_classifier, v_classifier, t_classifier)):   # order :272
                e.xval_counts(rows, row_labels, clf, counts[m, 0], counts[m, 1])
        if dist:
            from .shard import all_reduce_counts
            counts = all_reduce_counts(counts, dist)                                # ONE all-reduce
        if ragged:                                                                  # a class has as many rows as it has images
            n_label = self._ragged_n_label
        else:
            if getattr(self, "_n_label_key", None) != (C, S):
                self._n_label, self._n_label_key = torch.full((C,), S, dtype=torch.int32, device=dev), (C, S)
            n_label = self._n_label
        self.xval_counts = counts
        return e.fusion_weights(counts, n_label, tau)

    @torch.no_grad()
    def get_fusion_weight(self, eval_set_loader: Iterable, mm_classifier, v_classifier, t_classifier):
        """trainers/coop_mm_classifier.py:235-305: fusion weights for EXTERNALLY supplied classifiers [C, out].
        Encodes the exemplar set, then the same cross-validation F1 preference as forward_prompt with tau fixed at 10
        (:297).  The reference's [S, C, .] permuted feature layout (:277, :285-287) is undone before the row flatten,
        so rows are r = c*S + s with label c exactly as in forward_prompt; nothing is written to disk."""
        e, dev, dist = self.engine, self.device, self._dist
        C, S, D = len(self.tokenized_prompts), self.test_num_ins, e.spec.embed_dim
        rank, world = (dist.get_rank(), dist.get_world_size()) if dist else (0, 1)
        self.eval_feat4cls = torch.zeros((C, S, D), dtype=torch.float16, device=dev)
        self.eval_row_labels = self._ragged_n_label = None
        # (no all-gather of per-batch blocks here, so nothing bounds the classes of a round-robin batch)
        local_labels = [label for _, label, _ in self._exemplar_batches(eval_set_loader, rank, world, gathered=False)]   # :261-267
        local = torch.cat(local_labels) if local_labels else torch.zeros(0, dtype=torch.long, device=dev)
        clfs = [c.to(device=dev, dtype=torch.float16).contiguous() for c in (mm_classifier, v_classifier, t_classifier)]
        self.fusion_weight = self._xval_fusion_weight(local, *clfs, 10.0)
        self._has_features = False                           # (weights of external classifiers: no state a bank could describe)
        return self.fusion_weight

    @torch.no_grad()
    def forward(self, image, label=None, eval_set_loader=None, scale_no=None):
        """:294-364, evaluation branch: [B,3,R,R] -> [B,C] fp32; with cfg.EVAL_MODE == "all" [4,B,C], the four modes of :348-363 in
        runtime.ALL_MODES order (fusion, text, vision, multimodal), each plane bit-equal to what its own EVAL_MODE returns."""
        self._classifiers_or(eval_set_loader, NotImplementedError, "the training branch of CustomCLIP.forward (autograd) is out of scope; "
                             "pass eval_set_loader= to generate the classifiers")    # :341-342 (the features of `image` do not depend on it)
        B = image.shape[0]
        if self.SPLIT_FORWARD and 2 * self.SPLIT_MIN_HALF <= B <= self._split_cap() and self._split_keeps_bits(B):
            return self._forward_split(image)
        return self._forward_on(self.engine, image)

    __call__ = forward

    def _forward_on(self, engine: Engine, image, out=None):
        return self._head_on(engine, engine.encode_image(image, normalize=True), out)       # :305-307

    def _head_on(self, engine: Engine, image_features, out=None):
        mode = self.cfg.EVAL_MODE
        if mode not in ("text", "vision", "multimodal", "fusion", "all"):
            raise ValueError(f"unknown EVAL_MODE {mode}")
        kw = {} if out is None else {"out": out}             # (only the split forward hands an output slice in)
        if mode == "all":                                    # one pass over the head, four planes (ovmr_fused_logits_all)
            return engine.fused_logits_all(image_features, self.mm_classifier, self.visual_classifer,
                                           self.zero_shot_classifier, self.fusion_weight, **kw)
        return engine.fused_logits(image_features, self.mm_classifier, self.visual_classifer,
                                   self.zero_shot_classifier, self.fusion_weight, mode, **kw)

    # ------------------------------------------------------------------ one forward, its two halves in flight
    SPLIT_FORWARD = True          # forward(image) of an UNCHANGED test loop (one model(input) per batch, a host sync per batch): the batch's
    SPLIT_MIN_HALF = 64           # two halves run on two handles / streams, so that the partial last round of GEMM tiles of one half is filled
                                  # by the other's work -- what forward_batches does across batches, without asking the caller for the next batch.
                                  # Same rows bit for bit: a row's arithmetic does not depend on its batch as long as the head takes the
                                  # same implementation (_split_keeps_bits; tests/test_hip_configs.py).

    def _split_keeps_bits(self, B: int) -> bool:
        """The head runs as one launch or as GEMMs + softmax depending on the rows of a call (ovmr_head_plan), and the two may differ by one
        fp16 step in a logit: forward() splits a batch only where both halves take the implementation the whole batch takes, so that
        model(b), forward_batches and SPLIT_FORWARD = False agree bit for bit (e.g. 300 images against 10 000 classes run unsplit)."""
        C, e, half = len(self.tokenized_prompts), self.engine, (B + 1) // 2
        return e.head_plan(B, C) == e.head_plan(half, C) == e.head_plan(B - half, C)

    def _split_cap(self) -> int:
        return min(self.OVERLAP_MAX_BATCH, 2 * getattr(self.engine, "_reserve", (256,))[0])

    def _forward_split(self, image):
        self.engine.check_image(image)                       # refused before the batch is copied or the side stream is touched
        image = self.engine._dev(image)
        B, C = image.shape[0], len(self.tokenized_prompts)
        half = (B + 1) // 2
        cur = torch.cuda.current_stream(self.device)
        if not hasattr(self, "_split_stream"):
            self._split_stream = torch.cuda.Stream(self.device)
        st, twin = self._split_stream, self._twin()
        rows = (slice(None),) if self.cfg.EVAL_MODE == "all" else ()      # [4, B, C]: each handle writes its rows of every plane
        out = torch.empty(((4,) if rows else ()) + (B, C), dtype=torch.float32, device=self.device)
        st.wait_stream(cur)                                  # the image (and `out`) exist for the side stream
        with torch.cuda.stream(st):
            self._forward_on(twin, image[half:], out=out[rows + (slice(half, None),)])
        self._forward_on(self.engine, image[:half], out=out[rows + (slice(None, half),)])
        cur.wait_stream(st)
        image.record_stream(st)
        out.record_stream(st)
        return out

    # ------------------------------------------------------------------ ranked prediction (no counterpart in the reference's API)
    def _one_mode(self, what: str, noun: str = "a ranked prediction"):
        if self.cfg.EVAL_MODE == "all":
            raise ValueError(f"{what}: {noun} needs one mode; EVAL_MODE all yields four outputs per image "
                             "(set EVAL_MODE to fusion, text, vision or multimodal)")

    @torch.no_grad()
    def predict_topk(self, image, k: int, eval_set_loader=None):
        """forward(image) followed by ovmr_topk_rows on its output, on the same stream: (values fp32 [B, k], indices int64 [B, k]), the k
        most probable classes of every image, best first."""
        self._one_mode("predict_topk")
        return self._topk(self.forward(image, eval_set_loader=eval_set_loader), k)

    def predict_topk_batches(self, batches: Iterable, k: int, eval_set_loader=None, overlap: Optional[bool] = None, stable_inputs: bool = False):
        self._one_mode("predict_topk_batches")               # (raised by the call; the classifiers are the first next()'s, as in forward_batches)
        return super().predict_topk_batches(batches, k, eval_set_loader, overlap, stable_inputs)

    def _classifiers_or(self, eval_set_loader, error, text: str):
        """The classifiers exist, or are generated from eval_set_loader now (the files land while the caller goes on), or error(text)."""
        if self.mm_classifier is None:
            if eval_set_loader is None:
                raise error(text)
            self.forward_prompt(eval_set_loader, wait_files=False)

    def _before_outputs(self, what: str, eval_set_loader=None, one_mode: Optional[str] = None) -> int:
        if one_mode is not None:                             # (what `what` yields needs one mode: `one_mode` is the noun of the refusal)
            self._one_mode(what, one_mode)
        self._classifiers_or(eval_set_loader, NotImplementedError, "pass eval_set_loader= to generate the classifiers")
        return int(self.mm_classifier.shape[0])

    # ------------------------------------------------------------------ nearest exemplars (no counterpart in the reference's API)
    MAX_NEAREST = 32              # ovmr_nearest_rows (include/ovmr_hip_nearest.h)

    def _bank_view(self):
        """(bank [R, D] fp16, starts int64 [C + 1] on the device, starts as a host list, the longest class): the exemplar features class
        after class in label order -- the uniform [C, S, D] store viewed as [C S, D], the packed store as it is once its rows are in label
        order (load_bank and the edits leave it so; a ragged generation's loader order is sorted once and kept) -- and the prefix sum of
        the classes' shots.  Kept with the store it describes, so the packed store's class sizes are read back once per store."""
        src, lab = self.eval_feat4cls, getattr(self, "eval_row_labels", None)
        kept = self.__dict__.get("_nearest_bank")
        if kept is None or kept[0] is not src or kept[1] is not lab:
            if lab is None:
                C, S, D = src.shape
                bank, shots = src.reshape(C * S, D), [S] * C
            else:
                per_class = self._class_rows()
                bank, shots = torch.cat(per_class).contiguous(), [int(r.shape[0]) for r in per_class]
            starts = np.concatenate([[0], np.cumsum(shots, dtype=np.int64)]).tolist()
            kept = self._nearest_bank = (src, lab, bank, torch.tensor(starts, dtype=torch.int64).to(self.device), starts, max(shots, default=0))
        return kept[2:]

    def _exemplar_bank(self):
        """(bank [R, D] fp16, starts int64 [C + 1] on the device) of _bank_view()."""
        return self._bank_view()[:2]

    def _bank_starts_host(self):
        """(starts: list of C + 1 ints, the longest class) of _bank_view(), on the host."""
        return self._bank_view()[2:]

    def exemplar_rows(self, label_order_paths: Optional[Sequence[str]] = None):
        """(exemplars per class: C ints, the path of every bank row in label order: R strings, or None where there is no path per row).
        The paths are the model's own if it holds them (load_bank, the edits), else `label_order_paths`, dropped unless it counts R."""
        starts, own = self._bank_starts_host()[0], self._exemplar_paths
        paths = [p for ps in own for p in ps] if own is not None else list(label_order_paths or ())
        return [b - a for a, b in zip(starts, starts[1:])], paths if paths and len(paths) == starts[-1] else None

    @torch.no_grad()
    def nearest_exemplars(self, feats_or_image, k: int, classes=None):
        """The k exemplars nearest to every query, by h(query . exemplar) on the L2-normalised features (ovmr_nearest_rows, one fused
        launch pair on the current stream).  feats_or_image: image features [B, D] fp16 on the device (what engine.encode_image(...,
        normalize=True) returns), or an image batch [B, 3, R, R], which is encoded.  1 <= k <= 32.
        classes None: the whole bank -> (values fp32 [B, k], rows int64 [B, k], labels int64 [B, k]); rows index the bank's `features`
        (and its exemplar_paths), labels are the rows' classes.
        classes int64 [B] or [B, m] (host or device; [B] is m = 1): the nearest exemplars INSIDE each named class, one launch over B m
        queries -> three [B, m, k] tensors.  A class with fewer than k exemplars fills its tail with value -inf, row -1, label -1."""
        from . import runtime
        self._needs_state("nearest_exemplars")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= self.MAX_NEAREST:
            raise ValueError(f"nearest_exemplars: k must be an integer in [1, {self.MAX_NEAREST}], got {k!r}")
        k = int(k)
        bank, starts = self._exemplar_bank()
        if k > bank.shape[0]:
            raise ValueError(f"nearest_exemplars: k = {k} exceeds the bank's {bank.shape[0]} exemplar rows")
        feats = feats_or_image
        if isinstance(feats, (torch.Tensor, np.ndarray)) and feats.ndim == 4:
            feats = self.engine.encode_image(feats, normalize=True)
        runtime._want("nearest_exemplars", "feats_or_image", feats, (None, bank.shape[1]), torch.float16, self.device)
        B, C = feats.shape[0], starts.shape[0] - 1
        if classes is None:
            values, rows = runtime.nearest_rows(feats, bank, k)
            rows = rows.long()
            labels = torch.searchsorted(starts[1:], rows, right=True)
            return values, rows, torch.where(rows >= 0, labels, rows)
        runtime._want("nearest_exemplars", "classes", classes)
        classes = torch.as_tensor(classes)
        if classes.dtype != torch.int64 or classes.ndim not in (1, 2) or classes.shape[0] != B:
            raise ValueError(f"nearest_exemplars: classes must be int64 [{B}] or [{B}, m], got {classes.dtype} {list(classes.shape)}")
        runtime._want_range("nearest_exemplars", "classes", classes, 0, C, "class labels")
        classes = classes.to(self.device).reshape(B, -1)
        m = classes.shape[1]
        flat = classes.reshape(-1).clamp(0, C - 1)           # (device values are the caller's contract: clamped, so that nothing reads outside `starts`)
        ranges = torch.stack([starts[flat], starts[flat + 1]], 1).to(torch.int32)
        values, rows = runtime.nearest_rows(feats.repeat_interleave(m, 0) if m != 1 else feats, bank, k, ranges)
        rows = rows.long().view(B, m, k)
        return values.view(B, m, k), rows, torch.where(rows >= 0, classes[:, :, None].expand(B, m, k), rows)

    @torch.no_grad()
    def predict_explained(self, image, k: int, n: int, eval_set_loader=None):
        """predict_topk with its evidence: the image is encoded ONCE, the head and ovmr_topk_rows run on those features as in predict_topk,
        then nearest_exemplars(features, n, classes = the k predicted classes) on the same stream.  Returns (values fp32 [B, k], indices
        int64 [B, k], similarities fp32 [B, k, n], rows int64 [B, k, n]): the first two are predict_topk's, bit for bit; rows index the
        bank's features / exemplar_paths, -1 (similarity -inf) where a class has fewer than n exemplars."""
        self._one_mode("predict_explained")
        self._classifiers_or(eval_set_loader, ValueError, "predict_explained: the model has no classifiers yet (pass eval_set_loader=, or load_bank)")
        self._needs_state("predict_explained")
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= self.MAX_NEAREST:
            raise ValueError(f"predict_explained: n must be an integer in [1, {self.MAX_NEAREST}], got {n!r}")
        feats = self.engine.encode_image(image, normalize=True)
        values, indices = self._topk(self._head_on(self.engine, feats), k)
        sims, rows, _ = self.nearest_exemplars(feats, int(n), classes=indices)
        return values, indices, sims, rows

    # ------------------------------------------------------------------ auditing the reference bank (no counterpart in the reference's API)
    @torch.no_grad()
    def audit_bank(self, k: int = 5, classes=None, dup_threshold: float = 0.995, batch: int = 1024):
        """Every exemplar's nearest neighbours inside its own class (itself left out) and outside it, by h(row . row) on the view of
        _exemplar_bank() (uniform or packed store), and what follows from them.  1 <= k <= 32.  classes (host ints, None = all): the
        classes whose rows are audited, for instance freshly added ones; the search always sees the whole bank.  With N audited rows,
        a dict of device tensors:
          rows int64 [N], labels int64 [N]                   the audited bank rows, increasing, and their classes;
          in_sim fp32 [N, k], in_row int64 [N, k]            the class-mates nearest to the row: ONE launch over all N queries
                                                             (ovmr_neighbours_rows, range = the class, exclusion = the row itself,
                                                             max_range = the longest class); a full audit queries the bank itself, no copy;
          out_sim, out_row, out_label [N, k]                 the nearest rows of other classes (range = the bank, exclusion = the class),
                                                             the tiled launch pair in batches of `batch` queries on the same stream;
          suspect bool [N]                                   the closest image of another class is STRICTLY closer than the closest
                                                             class-mate (the library's order on values: NaN largest, -0 == +0); a class
                                                             of one image is never suspect;
          duplicate_of int64 [N]                             the better of the two first neighbours (larger value, then lower row) where
                                                             its similarity is >= dup_threshold (a NaN never is), else -1;
          class_suspects, class_duplicates int64 [C]         their counts per class.
        Missing neighbours are row -1, label -1, similarity -inf.  dup_threshold: an fp16 L2-normalised row scores a byte-identical copy at
        least 0.9990, so the default 0.995 always finds one; re-compressed near-duplicates need a lower value, which nobody has
        measured on real images.  Nothing synchronises with the host (the packed store's class sizes are read back once per store)."""
        from . import runtime
        self._needs_state("audit_bank")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= self.MAX_NEAREST:
            raise ValueError(f"audit_bank: k must be an integer in [1, {self.MAX_NEAREST}], got {k!r}")
        k = int(k)
        if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or int(batch) < 1:
            raise ValueError(f"audit_bank: batch must be a positive integer, got {batch!r}")
        if isinstance(dup_threshold, bool) or not isinstance(dup_threshold, (int, float, np.floating, np.integer)) or dup_threshold != dup_threshold:
            raise ValueError(f"audit_bank: dup_threshold must be a number, got {dup_threshold!r}")
        bank, starts, hstarts, longest = self._bank_view()
        R, C, dev = bank.shape[0], starts.shape[0] - 1, self.device
        if k > R:
            raise ValueError(f"audit_bank: k = {k} exceeds the bank's {R} exemplar rows")
        if classes is None:
            rows, queries = torch.arange(R, dtype=torch.int64, device=dev), bank
        else:
            which = np.unique(np.asarray(classes.cpu() if isinstance(classes, torch.Tensor) else classes).reshape(-1))
            if which.size and (not np.issubdtype(which.dtype, np.integer) or which.min() < 0 or which.max() >= C):
                raise ValueError(f"audit_bank: classes must be integer labels in [0, {C}), got {classes!r}")
            rows = torch.cat([torch.arange(hstarts[c], hstarts[c + 1], dtype=torch.int64) for c in which.tolist()]
                             + [torch.zeros(0, dtype=torch.int64)]).to(dev)
            queries = bank.index_select(0, rows)
        n = int(rows.shape[0])
        labels = torch.searchsorted(starts[1:], rows, right=True)
        own = torch.stack([starts[labels], starts[labels + 1]], 1).to(torch.int32)
        me = torch.stack([rows, rows + 1], 1).to(torch.int32)
        # inside the class: one wave per query; a class beyond the short launch's ceiling takes the tiled pair
        in_sim, in_row = runtime.neighbour_rows(queries, bank, k, own, me, longest if longest <= runtime.MAX_RANGE else 0)
        out_sim = torch.empty((n, k), dtype=torch.float32, device=dev)
        out_row = torch.empty((n, k), dtype=torch.int32, device=dev)
        for i in range(0, n, int(batch)):
            j = min(n, i + int(batch))
            runtime.neighbour_rows(queries[i:j], bank, k, None, own[i:j], 0, out=(out_sim[i:j], out_row[i:j]))
        in_row, out_row = in_row.long(), out_row.long()
        out_label = torch.where(out_row >= 0, torch.searchsorted(starts[1:], out_row.clamp(min=0), right=True), out_row)
        a, b = out_sim[:, 0], in_sim[:, 0]
        a_nan, b_nan = torch.isnan(a), torch.isnan(b)
        a_gt = (a_nan & ~b_nan) | (~a_nan & ~b_nan & (a > b))        # the library's order on values: NaN largest, -0 == +0
        b_gt = (b_nan & ~a_nan) | (~a_nan & ~b_nan & (b > a))
        has_in, has_out = in_row[:, 0] >= 0, out_row[:, 0] >= 0
        suspect = has_in & has_out & a_gt
        out_wins = has_out & (~has_in | a_gt | (~b_gt & (out_row[:, 0] < in_row[:, 0])))
        best_row = torch.where(out_wins, out_row[:, 0], in_row[:, 0])
        best_sim = torch.where(out_wins, a, b)
        duplicate_of = torch.where((best_row >= 0) & (best_sim >= float(dup_threshold)), best_row, torch.full_like(best_row, -1))
        ones = torch.ones_like(labels)
        class_suspects = torch.zeros(C, dtype=torch.int64, device=dev).index_add_(0, labels, ones * suspect)
        class_duplicates = torch.zeros(C, dtype=torch.int64, device=dev).index_add_(0, labels, ones * (duplicate_of >= 0))
        return {"rows": rows, "labels": labels, "in_sim": in_sim, "in_row": in_row, "out_sim": out_sim, "out_row": out_row,
                "out_label": out_label, "suspect": suspect, "duplicate_of": duplicate_of, "class_suspects": class_suspects,
                "class_duplicates": class_duplicates}

    @torch.no_grad()
    def load_classifiers(self, path: str):
        """Installs the classifiers of a mm_classifiers.pt written by forward_prompt (:276-285: text / vision / multimodal classifier
        [C, embed_dim] and fusion_weight [C, 3], all fp32; the three classifiers hold fp16 values, so .half() is exact) as forward_prompt
        leaves them: a later forward generates nothing.  Both handles of forward_batches read them from here.  visual_tokens.pt is not
        needed for inference and is not read.  Returns (mm_classifier, visual_classifer, fusion_weight)."""
        from . import checkpoint
        obj = checkpoint._torch_load(path)
        keys = ("text_classifier", "vision_classifier", "mm_classifier", "fusion_weight")
        if not isinstance(obj, dict) or any(not isinstance(obj.get(k), torch.Tensor) for k in keys):
            raise ValueError(f'"{path}" is not a mm_classifiers.pt: it must hold the tensors {keys}')
        C, D = len(self.tokenized_prompts), self.engine.spec.embed_dim
        for k in keys:
            want = (C, 3) if k == "fusion_weight" else (C, D)
            if tuple(obj[k].shape) != want:
                raise ValueError(f'"{path}": {k} is {tuple(obj[k].shape)}, this model has {C} classes of width {D} (expected {want})')
        self.wait_files()
        dev = self.device
        t, v, mm = (obj[k].to(dev).half().contiguous() for k in keys[:3])
        self.zero_shot_classifier = self.prompt_learner.zero_shot_classifier = t
        self.visual_classifer, self.mm_classifier = v, mm
        self.fusion_weight = obj["fusion_weight"].to(dev).float().contiguous()
        self.inference_text_initialized = torch.ones(C, dtype=torch.int32, device=dev)
        self._has_features = False                           # (the file holds no exemplar features: nothing to edit or to bank)
        return self.mm_classifier, self.visual_classifer, self.fusion_weight

    # ------------------------------------------------------------------ the reference bank and vocabulary edits (no counterpart in the reference)
    def _world(self) -> int:
        if self._dist is not None:
            return int(self._dist.get_world_size())
        import torch.distributed as dist
        return int(dist.get_world_size()) if dist.is_available() and dist.is_initialized() else 1

    def _needs_state(self, what: str):
        """The refusals every bank write and every edit share, before anything is encoded or copied."""
        if self._world() > 1:
            raise ValueError(f"{what}: not under a process group of more than one rank (a sharded rank holds only its own classes' exemplar features)")
        if self.mm_classifier is None:
            raise ValueError(f"{what}: the model has no classifiers yet (forward_prompt generates them, load_bank installs them)")
        if not self._has_features:
            raise ValueError(f"{what}: the model holds no exemplar features (load_classifiers installs classifiers only: generate, or load_bank)")

    def _join(self):
        """An edit starts from a quiet model: the file writer is joined and nothing of forward_batches is in flight on the side streams."""
        self.wait_files()
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def model_fingerprint(self) -> str:
        """bank.fingerprint of this model: spec, n_ctx, the prompt learner's state, a fixed set of CLIP tensors."""
        from . import bank
        pl = self.prompt_learner
        return bank.fingerprint(self.engine.spec, pl.n_ctx, pl.state_dict(), pl.clip_model.state_dict())

    def _ensure_capacity(self, num_classes: int):
        """ovmr_finalize sizes the engine's workspace by the reserve's third entry, max_classes.  A vocabulary that outgrows it re-finalises
        the engine and its twins (the handles of forward_batches) with that entry raised to `num_classes`, once, before the first launch of
        the edit or load.  This REALLOCATES the workspace (and rebuilds the derived weight layouts): callers have joined everything in
        flight (_join).  Nothing happens while the vocabulary fits."""
        e = self.engine
        res = tuple(getattr(e, "_reserve", (256, 256, 1024)))
        if num_classes <= res[2]:
            return
        e._reserve = (res[0], res[1], int(num_classes))
        e.finalize(*e._reserve)
        for t in self.__dict__.get("_twin_engines", {}).values():
            t._reserve = (t._reserve[0], t._reserve[1], int(num_classes))
            t.finalize(*t._reserve)

    def _class_rows(self):
        """The exemplar features as one [n_c, D] tensor per class, in label order (from the uniform [C, S, D] buffer or the packed rows)."""
        if getattr(self, "eval_row_labels", None) is None:
            return list(self.eval_feat4cls.unbind(0))
        order = torch.argsort(self.eval_row_labels.long(), stable=True)          # (a class's rows keep their order)
        return list(torch.split(self.eval_feat4cls[order], [int(n) for n in self._ragged_n_label.tolist()]))

    def _install_class_rows(self, per_class):
        """The exemplar store in its packed form: eval_feat4cls [R, D] class after class in label order, eval_row_labels int32 [R],
        _ragged_n_label int32 [C] -- what _xval_fusion_weight reads as they are."""
        dev = self.device
        shots = torch.tensor([int(r.shape[0]) for r in per_class], dtype=torch.int64)
        self.eval_feat4cls = torch.cat(per_class).contiguous()
        self.eval_row_labels = torch.repeat_interleave(torch.arange(len(per_class), dtype=torch.int32), shots).to(dev)
        self._ragged_n_label = shots.to(device=dev, dtype=torch.int32)

    def _recount(self):
        """The cross-validation over ALL packed rows and all classifier rows (ovmr_xval_counts: milliseconds for a whole vocabulary), then
        the fusion weights: xval_counts and fusion_weight are a function of the state, whatever the edits that led to it."""
        nothing = torch.zeros(0, dtype=torch.long, device=self.device)
        self.fusion_weight = self._xval_fusion_weight(nothing, self.mm_classifier, self.visual_classifer, self.zero_shot_classifier,
                                                      float(self.cfg.EVAL_TAU))

    @torch.no_grad()
    def bank_state(self) -> dict:
        """Every field of a reference bank (ovmr_amd/bank.py FIELDS) from the model's state, tensors on the model's device; the exemplar
        features packed class after class in label order, whichever layout the generation left them in."""
        from . import bank
        self._needs_state("bank_state")
        pl, per_class = self.prompt_learner, self._class_rows()
        paths = self._exemplar_paths
        return {"format": bank.BANK_FORMAT, "fingerprint": self.model_fingerprint(), "n_ctx": int(pl.n_ctx),
                "embed_dim": int(self.engine.spec.embed_dim), "tau": float(self.cfg.EVAL_TAU), "num_shots_cap": int(self.cfg.DATASET.NUM_SHOTS),
                "classnames": None if self.classnames is None else list(self.classnames),
                "exemplar_paths": None if paths is None else [p for ps in paths for p in ps],
                "tokenized_prompts": pl._tokenized_host.clone(),
                "shots": torch.tensor([int(r.shape[0]) for r in per_class], dtype=torch.int32),
                "features": torch.cat(per_class).contiguous(),
                "mm_classifier": self.mm_classifier, "vision_classifier": self.visual_classifer, "text_classifier": self.zero_shot_classifier,
                "visual_tokens": self.visual_tokens, "xval_counts": self.xval_counts, "fusion_weight": self.fusion_weight}

    @torch.no_grad()
    def save_bank(self, path: str, exemplar_paths: Optional[Sequence[str]] = None):
        """Writes the reference bank of this model (ovmr_amd/bank.py) to `path`: valid once classifiers exist and the exemplar features they
        were generated from are present -- refused after load_classifiers, and under a process group of more than one rank.  The state is
        snapshotted here and written inline, under a scratch name that is moved into place whole.  exemplar_paths: one path per exemplar
        row in label order, for provenance (the runner fills it)."""
        from . import bank
        self._needs_state("save_bank")
        self.wait_files()
        state = self.bank_state()
        if exemplar_paths is not None:
            if len(exemplar_paths) != state["features"].shape[0]:
                raise ValueError(f"save_bank: {len(exemplar_paths)} exemplar paths for {state['features'].shape[0]} exemplar rows")
            state["exemplar_paths"] = [str(p) for p in exemplar_paths]
        bank.write(path, {k: (v.detach().cpu().contiguous() if isinstance(v, torch.Tensor) else v) for k, v in state.items()})

    @torch.no_grad()
    def save_classifiers(self):
        """mm_classifiers.pt / visual_tokens.pt of the model's present state into cfg.OUTPUT_DIR, as forward_prompt writes them (the same
        bytes for the same state): for a model whose vocabulary was loaded from a bank or edited."""
        if self.mm_classifier is None:
            raise ValueError("save_classifiers: the model has no classifiers yet")
        self._write_files()()
        self.wait_files()

    @torch.no_grad()
    def load_bank(self, path: str, bank_read: Optional[dict] = None):
        """Installs the vocabulary and every tensor of a reference bank: a superset of load_classifiers.  A later forward, forward_batches
        or predict_topk* generates nothing and decodes no exemplar, and the model can be edited (add / replace / remove_classes).  The bank
        REPLACES the model's class list: a model built for another class list or class count loads any bank of its own model fingerprint.
        Another n_ctx or width, a newer format, a file that is not a bank and a fingerprint mismatch are ValueErrors naming file and field
        (bank.read).  If cfg.EVAL_TAU differs from the bank's tau the fusion weights are recomputed from the stored counters
        (Engine.fusion_weights: exact).  A ragged bank whose longest class needs more aggregator rows than the engine's agg_max_len still
        loads: inference does not run the aggregator.  A vocabulary beyond the engine's reserve re-finalises it (_ensure_capacity).
        bank_read: what bank.read(path) returned, for a caller that has read the file already (the runner needs its class names first).
        Returns (mm_classifier, visual_classifer, fusion_weight)."""
        from . import bank
        if self._world() > 1:
            raise ValueError("load_bank: not under a process group of more than one rank")
        e, pl, dev = self.engine, self.prompt_learner, self.device
        b = bank.read(path) if bank_read is None else bank_read
        bank.check_model(path, b, pl.n_ctx, e.spec.embed_dim, e.spec.context_length, self.model_fingerprint())
        self._join()
        C = b["tokenized_prompts"].shape[0]
        self._ensure_capacity(C)
        pl.install_vocabulary(b["tokenized_prompts"])
        self.tokenized_prompts = pl.tokenized_prompts
        self.classnames = None if b["classnames"] is None else list(b["classnames"])
        self.mm_classifier = b["mm_classifier"].to(dev)
        self.visual_classifer = b["vision_classifier"].to(dev)
        self.zero_shot_classifier = pl.zero_shot_classifier = b["text_classifier"].to(dev)
        self.visual_tokens = b["visual_tokens"].to(dev)
        self.xval_counts = b["xval_counts"].to(dev)
        self.inference_text_initialized = torch.ones(C, dtype=torch.int32, device=dev)
        shots = [int(n) for n in b["shots"].tolist()]
        self._install_class_rows(list(torch.split(b["features"].to(dev), shots)))
        paths = b["exemplar_paths"]
        self._exemplar_paths = None if paths is None else [list(paths[a - n:a]) for a, n in zip(np.cumsum(shots).tolist(), shots)]
        if float(b["tau"]) == float(self.cfg.EVAL_TAU):
            self.fusion_weight = b["fusion_weight"].to(dev)
        else:
            self.fusion_weight = e.fusion_weights(self.xval_counts, self._ragged_n_label, float(self.cfg.EVAL_TAU))
        self._has_features = True
        return self.mm_classifier, self.visual_classifer, self.fusion_weight

    # ---- edits
    def _edit_labels(self, what: str, labels_or_names) -> List[int]:
        """Class labels from labels or class names: unknown names, labels out of range and classes named twice are refused."""
        C = len(self.tokenized_prompts)
        if isinstance(labels_or_names, (torch.Tensor, np.ndarray)):
            labels_or_names = torch.as_tensor(labels_or_names).tolist()
        if isinstance(labels_or_names, (str, int)):
            labels_or_names = [labels_or_names]
        out = []
        for x in labels_or_names:
            if isinstance(x, str):
                if self.classnames is None or x not in self.classnames:
                    raise ValueError(f"{what}: unknown class name {x!r}" + (" (this model's vocabulary was given as token rows: it has no names)"
                                                                           if self.classnames is None else ""))
                x = self.classnames.index(x)
            x = int(x)
            if not 0 <= x < C:
                raise ValueError(f"{what}: label {x} outside [0, {C})")
            if x in out:
                raise ValueError(f"{what}: class {x} is named twice")
            out.append(x)
        if not out:
            raise ValueError(f"{what}: no class named")
        return out

    def _new_token_rows(self, what: str, classnames_or_ids):
        """(token rows [K, context_length] on the host, the K names or None) of classes to append: refused when one of them is in the
        vocabulary already (or twice in the call), when names come to a model without a tokenizer, or token rows to a model with names."""
        pl = self.prompt_learner
        L = self.engine.spec.context_length
        if isinstance(classnames_or_ids, (torch.Tensor, np.ndarray)):
            rows, names = torch.as_tensor(classnames_or_ids).long().cpu(), None
            if rows.dim() != 2 or rows.shape[1] != L or not rows.shape[0]:
                raise ValueError(f"{what}: token rows must be [K, {L}] with K >= 1, got {list(rows.shape)}")
            if self.classnames is not None:
                raise ValueError(f"{what}: this model's vocabulary has class names: pass names, not token rows")
        else:
            names = [classnames_or_ids] if isinstance(classnames_or_ids, str) else list(classnames_or_ids)
            if not names:
                raise ValueError(f"{what}: no class named")
            if self.classnames is None and pl.tokenizer is None:
                raise ValueError(f"{what}: class names given to a model that has no tokenizer (it was built from token rows: pass token rows [K, {L}])")
            if self.classnames is not None:
                for n in names:
                    if n in self.classnames:
                        raise ValueError(f"{what}: class name {n!r} is in the vocabulary already (label {self.classnames.index(n)})")
            rows = pl.tokenize_names(names)
            if self.classnames is None:
                names = None                                                      # (the old classes have none: the list stays absent)
        have = {r.numpy().tobytes(): i for i, r in enumerate(pl._tokenized_host)}
        for k, r in enumerate(rows):
            key = r.numpy().tobytes()
            if key in have:
                where = f"label {have[key]}" if have[key] >= 0 else "given twice"
                raise ValueError(f"{what}: the prompt of new class {k}" + (f" ({names[k]!r})" if names else "") + f" is in the vocabulary already ({where})")
            have[key] = -1
        return rows, names

    def _class_row_limit(self) -> int:
        return max(128, int(getattr(self.engine, "_options", {}).get("agg_max_len", 128))) - self.prompt_learner.n_ctx

    def _check_class_shots(self, what: str, shots):
        cap = int(self.cfg.DATASET.NUM_SHOTS)
        for k, n in enumerate(int(x) for x in shots):
            if n > cap:
                raise ValueError(f"{what}: class {k} of the loader brings {n} exemplars, more than DATASET.NUM_SHOTS = {cap}")
            if n > self._class_row_limit():
                raise ValueError(f"{what}: class {k} of the loader needs n_ctx + {n} aggregator rows, the engine takes {self._class_row_limit() + self.prompt_learner.n_ctx} "
                                 "(engine option agg_max_len: set by a larger DATASET.NUM_SHOTS at construction)")

    def _check_edit(self, what: str, K: int, eval_set_loader):
        """The refusals of an edit that do not depend on the classes named: all before anything is encoded or copied."""
        self._needs_state(what)
        if self.aug_times > 1:
            raise ValueError(f"{what}: vocabulary edits do not take DATALOADER.K_TRANSFORMS > 1")
        n = getattr(eval_set_loader, "shots", None)
        if isinstance(n, (torch.Tensor, np.ndarray)) and n.ndim == 1:              # a ragged loader says up front what every class brings
            if len(n) != K:
                raise ValueError(f"{what}: the loader describes {len(n)} classes, {K} are named")
            self._check_class_shots(what, torch.as_tensor(n).tolist())

    def _relabelled(self, what: str, eval_set_loader, target: List[int]):
        """The edit's loader yields its classes labelled 0 ... K - 1: its batches with the labels those classes have in the vocabulary."""
        table = torch.tensor(target, dtype=torch.long)
        for batch in eval_set_loader:
            label = batch["label"]
            if label.numel() and (int(label.min()) < 0 or int(label.max()) >= len(target)):
                raise ValueError(f"{what}: the loader's labels must lie in [0, {len(target)}), got {int(label.min())} ... {int(label.max())}")
            if "shots" in batch:
                self._check_class_shots(what, batch["shots"].tolist())
            out = dict(batch)
            out["label"] = table.to(label.device)[label.long()]
            yield out

    def _regenerate(self, what: str, target: List[int], eval_set_loader) -> Dict[int, torch.Tensor]:
        """Rows of the classes `target` (their vocabulary labels, in the order of the loader's labels 0 ... K - 1) from the loader's batches:
        per batch exactly the body of _generate_local with streamed text rows -- encode, PromptLearner.forward, ONE get_mm_v_feats pass with
        the batch's own zero-shot ids -- written at their labels into the model's buffers (which the caller has sized; every other row is
        left alone).  Returns each class's exemplar features [n_c, D]."""
        keep: list = []
        self.inference_text_initialized.index_fill_(0, torch.tensor(target, dtype=torch.long, device=self.device), 0)
        streamed, rows = self._text_streamed, getattr(self, "_text_rows", None)
        self._text_streamed, self._text_rows = True, self.zero_shot_classifier
        try:
            self._generate_local(self._relabelled(what, eval_set_loader, target), keep=keep)
        finally:
            self._text_streamed, self._text_rows = streamed, rows
        got: Dict[int, torch.Tensor] = {}
        for feats, labels, shots in keep:
            for c, r in zip(labels.tolist(), torch.split(feats, [int(n) for n in shots])):
                if int(c) in got:
                    raise ValueError(f"{what}: the loader brings class {target.index(int(c))} in more than one run of rows")
                got[int(c)] = r
        missing = [k for k, c in enumerate(target) if c not in got]
        if missing:
            raise ValueError(f"{what}: the loader brings no exemplar for class {missing[0]}" + (f" and {len(missing) - 1} more" if len(missing) > 1 else ""))
        return got

    _EDITED = ("mm_classifier", "visual_classifer", "zero_shot_classifier", "visual_tokens", "inference_text_initialized", "eval_feat4cls",
               "eval_row_labels", "_ragged_n_label", "fusion_weight", "xval_counts", "classnames", "_exemplar_paths", "tokenized_prompts")

    def _edit(self, what: str, change):
        """Runs change() on a quiet model; if it raises, the model is what it was (every edit builds new tensors or works on copies)."""
        pl = self.prompt_learner
        self._join()
        before = {k: getattr(self, k, None) for k in self._EDITED}
        vocabulary, embedded = pl._tokenized_host, pl.prompt_tokens
        try:
            change()
        except BaseException:
            for k, v in before.items():
                setattr(self, k, v)
            pl.install_vocabulary(vocabulary, prompt_tokens=embedded)
            pl.zero_shot_classifier = self.zero_shot_classifier
            raise
        return self.mm_classifier, self.visual_classifer, self.fusion_weight

    def _set_vocabulary(self, token_rows, prompt_tokens, classnames):
        pl = self.prompt_learner
        pl.install_vocabulary(token_rows, prompt_tokens=prompt_tokens)
        self.tokenized_prompts, self.classnames = pl.tokenized_prompts, classnames

    @torch.no_grad()
    def add_classes(self, classnames_or_token_ids, eval_set_loader: Iterable, exemplar_paths=None):
        """Appends K classes -- names, or token rows [K, context_length] for a model built from token rows -- with the labels C ... C + K - 1.
        `eval_set_loader` yields the NEW classes only, labelled 0 ... K - 1, uniform (NUM_SHOTS rows per class) or with "shots".  Only the
        new classes are encoded and generated (_regenerate: the loop of forward_prompt); no classifier row or visual token of an old class
        is recomputed; then the cross-validation runs over all exemplar rows and all C + K classifier rows (_recount).  A vocabulary beyond
        the engine's reserve re-finalises it first (_ensure_capacity: reallocates the workspace).  exemplar_paths: K lists of paths, one
        per row of each new class (provenance for save_bank).  Refusals are one-line ValueErrors before anything is encoded or copied; an
        error later leaves the model as it was.  Returns (mm_classifier, visual_classifer, fusion_weight)."""
        what = "add_classes"
        self._needs_state(what)
        rows, names = self._new_token_rows(what, classnames_or_token_ids)
        K = rows.shape[0]
        self._check_edit(what, K, eval_set_loader)

        def change():
            e, pl, dev = self.engine, self.prompt_learner, self.device
            C, D = len(self.tokenized_prompts), e.spec.embed_dim
            self._ensure_capacity(C + K)
            per_class, paths = self._class_rows(), self._exemplar_paths
            new_tokens = e.embed_tokens(rows.to(dev))
            self._set_vocabulary(torch.cat([pl._tokenized_host, rows]), torch.cat([pl.prompt_tokens, new_tokens]),
                                 None if names is None else self.classnames + names)
            f16 = dict(dtype=torch.float16, device=dev)
            self.mm_classifier = torch.cat([self.mm_classifier, torch.zeros((K, D), **f16)])
            self.visual_classifer = torch.cat([self.visual_classifer, torch.zeros((K, D), **f16)])
            self.zero_shot_classifier = pl.zero_shot_classifier = torch.cat([self.zero_shot_classifier, torch.zeros((K, D), **f16)])
            self.visual_tokens = torch.cat([self.visual_tokens, torch.ones((K, pl.n_ctx, D), **f16)])
            self.inference_text_initialized = torch.cat([self.inference_text_initialized, torch.zeros(K, dtype=torch.int32, device=dev)])
            target = list(range(C, C + K))
            got = self._regenerate(what, target, eval_set_loader)
            self._install_class_rows(per_class + [got[c] for c in target])
            self._exemplar_paths = None if paths is None or exemplar_paths is None else paths + [list(p) for p in exemplar_paths]
            self._recount()

        return self._edit(what, change)

    @torch.no_grad()
    def replace_classes(self, labels_or_names, eval_set_loader: Iterable, exemplar_paths=None):
        """New exemplars for existing classes (labels or names; the names stay): the loader yields those classes only, labelled 0 ... K - 1 in
        the order they are named here, and their counts may change.  Their rows are regenerated in place, their features replaced, and the
        cross-validation is redone over everything; every other class's rows and tokens stay bit for bit.  Refusals and return as add_classes."""
        what = "replace_classes"
        self._needs_state(what)
        target = self._edit_labels(what, labels_or_names)
        self._check_edit(what, len(target), eval_set_loader)

        def change():
            pl = self.prompt_learner
            per_class, paths = self._class_rows(), self._exemplar_paths
            for k in ("mm_classifier", "visual_classifer", "zero_shot_classifier", "visual_tokens", "inference_text_initialized"):
                setattr(self, k, getattr(self, k).clone())                           # (the rows are written in place: into copies)
            pl.zero_shot_classifier = self.zero_shot_classifier
            got = self._regenerate(what, target, eval_set_loader)
            for c in target:
                per_class[c] = got[c]
            self._install_class_rows(per_class)
            if paths is not None and exemplar_paths is not None:
                paths = list(paths)
                for c, p in zip(target, exemplar_paths):
                    paths[c] = list(p)
                self._exemplar_paths = paths
            else:
                self._exemplar_paths = None
            self._recount()

        return self._edit(what, change)

    @torch.no_grad()
    def remove_classes(self, labels_or_names):
        """Drops classes (labels or names) everywhere -- vocabulary, classifier rows, visual tokens, exemplar features -- relabels the
        survivors in order and redoes the cross-validation over what is left.  Removing every class is refused.  Return as add_classes."""
        what = "remove_classes"
        self._needs_state(what)
        gone = set(self._edit_labels(what, labels_or_names))
        C = len(self.tokenized_prompts)
        if len(gone) == C:
            raise ValueError(f"{what}: removing every class leaves no vocabulary")
        if self.aug_times > 1:
            raise ValueError(f"{what}: vocabulary edits do not take DATALOADER.K_TRANSFORMS > 1")

        def change():
            pl, dev = self.prompt_learner, self.device
            stay = [c for c in range(C) if c not in gone]
            idx = torch.tensor(stay, dtype=torch.long)
            per_class, paths = self._class_rows(), self._exemplar_paths
            on = idx.to(dev)
            self._set_vocabulary(pl._tokenized_host[idx], pl.prompt_tokens[on],
                                 None if self.classnames is None else [self.classnames[c] for c in stay])
            for k in ("mm_classifier", "visual_classifer", "zero_shot_classifier", "visual_tokens", "inference_text_initialized"):
                setattr(self, k, getattr(self, k)[on].contiguous())
            pl.zero_shot_classifier = self.zero_shot_classifier
            self._install_class_rows([per_class[c] for c in stay])
            self._exemplar_paths = None if paths is None else [paths[c] for c in stay]
            self._recount()

        return self._edit(what, change)

    @torch.no_grad()
    def forward_batches(self, batches: Iterable, eval_set_loader=None, overlap: Optional[bool] = None, stable_inputs: bool = False):
        """The model calls of the evaluation loop (dassl's test(): one forward per test batch, trainers' model_inference),
        software-pipelined: yields forward(image) for every image batch of `batches`, in order and bit-identical to calling
        forward on each, but with TWO batches in flight -- batch i on one handle and stream, batch i + 1 on a twin handle and a
        second stream -- so that the partial last round of tiles of one batch's launches (batch 256: 197 row tiles x 3 column
        tiles = 2.31 rounds of the 256 CUs on the N = 768 GEMMs) is filled by the other batch's work.  The output of batch i
        is handed over after batch i + 1 has been enqueued; using it on the current stream is ordered after its computation.

        overlap: None = for batches of at most OVERLAP_MAX_BATCH images (measured, ViT-B/16: 256 images 27.7 k -> 29.7 k img/s,
        768 images 30.7 k -> 28.7 k; profiles/r03t_two_stream.log, r03u_two_stream_sweep.log).  stable_inputs: the caller guarantees that a batch's
        tensor is not overwritten before its output has been handed over (a resident data set); otherwise each batch is first
        copied on the current stream, so that loaders which recycle their device buffers (loader.PipelinedFolderLoader)
        stay correct."""
        return self.output_batches(batches, eval_set_loader, overlap, stable_inputs)


class ZeroshotCLIP(_TwoInFlight):
    """trainers/zsclip.py:32-60 (BASELINE config 1): prompts -> text features; raw logits.
    `tokenized_prompts`: LongTensor [C, 77] -- clip.tokenize of CUSTOM_TEMPLATES[dataset].format(classname) (:42-45; tokenize() above with a
    BPE tokenizer produces them from names)."""

    TRAINER = "ZeroshotCLIP"

    def __init__(self, clip_model: CLIPModel, tokenized_prompts: torch.Tensor, n_ctx: int = 2, reserve=(256, 256, 1024)):
        self.clip_model = clip_model
        self.engine = e = clip_model.engine(n_ctx)
        self.device = e.device
        if not hasattr(e, "_pl_loaded"):                   # (the engine's handle also serves CustomCLIP: it wants the aggregator's weights)
            self._pl_state = {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(clip_model.spec, n_ctx, 0).items()}
            e.load_state_dict({}, self._pl_state)
            e._pl_loaded = True
        if not e.finalized:
            e._reserve = tuple(reserve)
            e.finalize(*reserve)
        self.tokenized_prompts = tokenized_prompts
        self.text_features = self._text_features(e, tokenized_prompts)

    def _text_features(self, e: Engine, tokenized_prompts: torch.Tensor) -> torch.Tensor:
        return e.encode_text_ids(tokenized_prompts, normalize=1)                    # :47-50

    @classmethod
    def from_classnames(cls, clip_model: CLIPModel, classnames: Sequence[str], dataset_name: str, tokenizer=None, **kw):
        """build_model from class names (:42-50; ZeroshotCLIP2: :85-96): every template of `dataset_name` (ovmr_amd.templates) is
        formatted with `c.replace("_", " ")` and tokenised with `tokenizer` (default: default_tokenizer()).  Unknown dataset names are
        refused (KeyError listing the known ones) before anything is tokenised."""
        from . import templates
        temps = templates.templates_for(cls.TRAINER, dataset_name)
        if tokenizer is None:
            tokenizer = default_tokenizer()
        texts = [templates.prompts(t, classnames) for t in temps]
        if cls.TRAINER == "ZeroshotCLIP":
            print(f"Prompts: {texts[0]}")                                        # :44
        ids = torch.stack([tokenize(p, tokenizer, clip_model.context_length) for p in texts])   # [T, C, 77], template-major
        return cls(clip_model, ids[0] if cls.TRAINER == "ZeroshotCLIP" else ids, **kw)

    def _twin_state(self):
        pl = getattr(self, "_pl_state", None)
        if pl is None:
            pl = {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(self.clip_model.spec, self.engine.n_ctx, 0).items()}
        return self.clip_model.state_dict(), pl

    def _forward_on(self, engine: Engine, image, out=None):
        f = engine.encode_image(image, normalize=True)                              # :56-57
        return engine.zeroshot_logits(f, self.text_features)                        # :58-59

    def model_inference(self, image):
        return self._forward_on(self.engine, image)

    # ranked prediction (no counterpart in the reference's API); eval_set_loader is accepted for CustomCLIP's signature and not read
    @torch.no_grad()
    def predict_topk(self, image, k: int, eval_set_loader=None):
        """model_inference(image) followed by ovmr_topk_rows on its logits, on the same stream: (values fp32 [B, k], indices int64 [B, k])."""
        return self._topk(self.model_inference(image), k)

    def _before_outputs(self, what: str, eval_set_loader=None, one_mode: Optional[str] = None) -> int:
        return int(self.text_features.shape[0])              # (the text classifier exists since __init__, and there is one mode)

    def inference_batches(self, batches: Iterable, overlap: Optional[bool] = None, stable_inputs: bool = False):
        """model_inference for every image batch of the test loop (Dassl.pytorch/dassl/engine/trainer.py:461-482), in order and bit-identical
        to calling it per batch, two batches in flight on two handles / streams (as CustomCLIP.forward_batches)."""
        return self.output_batches(batches, None, overlap, stable_inputs)


class ZeroshotCLIP2(ZeroshotCLIP):
    """trainers/zsclip.py:63-99, prompt ensembling.  `tokenized_prompts`: LongTensor [T, C, 77], template-major -- clip.tokenize of every
    template of ovmr_amd.templates.templates_for("ZeroshotCLIP2", dataset) formatted with every class name (from_classnames builds it).
    The text features are the ensembled classifier of ovmr_encode_text_ensemble (all templates of a chunk of classes in ONE tower pass,
    the reference's fp16 rounding points of :88-96); model_inference / inference_batches are ZeroshotCLIP's."""

    TRAINER = "ZeroshotCLIP2"

    def _text_features(self, e: Engine, tokenized_prompts: torch.Tensor) -> torch.Tensor:
        if tokenized_prompts.dim() != 3:
            raise ValueError(f"ZeroshotCLIP2 takes token ids [templates, classes, context_length], got {tuple(tokenized_prompts.shape)}")
        print(f"Prompt ensembling (n={tokenized_prompts.shape[0]})")                # :85-86
        return e.encode_text_ensemble(tokenized_prompts)


class LinearProbe(_TwoInFlight):
    """lpclip/feat_extractor.py + lpclip/linear_probe.py: a logistic regression on image features, fitted on the device (ovmr_amd.probe,
    csrc/probe.hip) and evaluated through the engine's batch path.  The reference probes the raw features of its RN50 tower; this path
    probes the L2-NORMALISED features of the ViT tower -- what encode_image(normalize=True) returns and what a reference bank holds
    (DESIGN.md section 6).  Outputs are fp32 [B, C] scores x W^T + b of ovmr_probe_logits, the GEMM the fit itself evaluates."""

    TRAINER = "LinearProbe"
    TOL = 1e-4                    # scikit-learn's default gtol
    MAX_ITER = 1000               # lpclip/linear_probe.py:57

    def __init__(self, clip_model: CLIPModel, classnames: Sequence[str], n_ctx: int = 2, reserve=(256, 256, 1024)):
        self.clip_model = clip_model
        self.engine = e = clip_model.engine(n_ctx)
        self.device = e.device
        if not hasattr(e, "_pl_loaded"):                   # (as ZeroshotCLIP: the handle wants the aggregator's weights)
            self._pl_state = {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(clip_model.spec, n_ctx, 0).items()}
            e.load_state_dict({}, self._pl_state)
            e._pl_loaded = True
        if not e.finalized:
            e._reserve = tuple(reserve)
            e.finalize(*reserve)
        self.classnames = [str(n) for n in classnames]
        self.W = self.b = self.state = None

    _twin_state = ZeroshotCLIP._twin_state

    def _labels_of(self, shots) -> torch.Tensor:
        shots = torch.as_tensor(shots, dtype=torch.int64).reshape(-1).cpu()
        if len(shots) != len(self.classnames) or bool((shots < 0).any()):
            raise ValueError(f"LinearProbe: shots must hold one count per class ({len(self.classnames)}), none negative, got {len(shots)} entries")
        return torch.repeat_interleave(torch.arange(len(shots)), shots)

    @torch.no_grad()
    def fit_features(self, features_f16: torch.Tensor, shots, c: float = 1.0, tol: Optional[float] = None, max_iter: Optional[int] = None,
                     install: bool = True):
        """Fits the probe at strength c on exemplar features packed class after class: features_f16 [R, D] (any float dtype; a bank's
        `features`), shots [C] rows per class.  The features are converted to fp32 ONCE and stay on the device.  -> probe.LinearProbeState
        (installed unless install=False)."""
        from . import probe
        labels = self._labels_of(shots)
        D = self.engine.spec.embed_dim
        if features_f16.dim() != 2 or tuple(features_f16.shape) != (len(labels), D):
            raise ValueError(f"LinearProbe.fit_features: features must be of shape [{len(labels)}, {D}] (sum(shots) rows of embed_dim), got "
                             f"{list(features_f16.shape)}")
        if len(labels) == 0:
            raise ValueError("LinearProbe.fit_features: no exemplar row to fit on")
        with torch.cuda.device(self.device):
            x = features_f16.to(self.device).float().contiguous()
            y = labels.to(self.device)
            tol, max_iter = self.TOL if tol is None else tol, self.MAX_ITER if max_iter is None else max_iter
            r = probe.fit(probe.device_loss_grad(x, y), len(self.classnames), D, float(c), tol=tol, max_iter=max_iter, device=self.device)
        state = probe.LinearProbeState(r.W, r.b, c, tol, r.n_iter, r.converged, self.classnames, torch.as_tensor(shots), None)
        state.loss, state.n_eval = r.loss, r.n_eval
        if install:
            self.install(state)
        return state

    @torch.no_grad()
    def encode_loader(self, loader: Iterable):
        """Every batch of a loader through encode_image(normalize=True), in the order of the walk -> (features fp16 [R, D] on the device,
        labels int64 [R] on the host)."""
        feats, labels = [], []
        for batch in loader:
            image = CustomCLIP._batch_images(batch, self.device)
            feats.append(self.engine.encode_image(image, normalize=True).clone())
            labels.append(batch["label"].reshape(-1).to(torch.int64).cpu())
        if not feats:
            raise ValueError("LinearProbe: the loader holds no batch")
        labels = torch.cat(labels)
        C = len(self.classnames)
        if bool(((labels < 0) | (labels >= C)).any()):
            raise ValueError(f"LinearProbe: labels must lie in [0, {C}), got values from {int(labels.min())} to {int(labels.max())}")
        return torch.cat(feats), labels

    def exemplar_features(self, eval_set_loader: Iterable):
        """The one loader walk MM_CLS_OP uses for its exemplars (encode_loader); the rows are then packed class after class, a class's
        rows in the order of the walk -- a reference bank's layout.  -> (features fp16 [R, D] on the device, shots int64 [C] on the host)."""
        feats, labels = self.encode_loader(eval_set_loader)
        order = torch.sort(labels, stable=True).indices
        return feats[order.to(self.device)], torch.bincount(labels, minlength=len(self.classnames))

    def fit_exemplars(self, eval_set_loader: Iterable, c: float = 1.0, **kw):
        """exemplar_features + fit_features: the probe of the images an eval-set loader yields."""
        feats, shots = self.exemplar_features(eval_set_loader)
        return self.fit_features(feats, shots, c, **kw)

    def install(self, state):
        """Makes a fitted or read probe.LinearProbeState the model's classifier (held to the model by class count and embed_dim)."""
        C, D = len(self.classnames), self.engine.spec.embed_dim
        if tuple(state.W.shape) != (C, D):
            raise ValueError(f"LinearProbe.install: the probe's W is {list(state.W.shape)}, this model has {C} classes and embed_dim {D}")
        with torch.cuda.device(self.device):
            self.W, self.b = state.W.to(self.device).contiguous(), state.b.to(self.device).contiguous()
        self.state = state

    def _forward_on(self, engine: Engine, image, out=None):
        from . import runtime
        if self.W is None:
            raise RuntimeError("LinearProbe has no probe yet: fit_exemplars / fit_features / install come first")
        f = engine.encode_image(image, normalize=True)
        return runtime.probe_logits(f.float(), self.W, self.b)

    def model_inference(self, image):
        return self._forward_on(self.engine, image)

    @torch.no_grad()
    def predict_topk(self, image, k: int, eval_set_loader=None):
        """model_inference(image) followed by ovmr_topk_rows on its scores: (values fp32 [B, k], indices int64 [B, k])."""
        return self._topk(self.model_inference(image), k)

    def _before_outputs(self, what: str, eval_set_loader=None, one_mode: Optional[str] = None) -> int:
        if self.W is None:
            if eval_set_loader is None:
                raise RuntimeError(f"{what}: LinearProbe has no probe yet and no exemplar loader to fit one from")
            self.fit_exemplars(eval_set_loader)
        return len(self.classnames)
