"""The reference bank: one file that holds everything a vocabulary edit or a later prediction run needs, and nothing that needs the data
set ("Editing a generated vocabulary").  No counterpart in the reference: its mm_classifiers.pt holds neither the
class names nor anything a fusion weight could be recomputed from.

`reference_bank.pt` is one torch.save of a dict of host tensors and plain values (FIELDS below): the vocabulary (token rows, class names
where the model has them), the L2-normalised exemplar features packed class after class in label order with the per-class counts, the three
classifiers, the visual tokens, the cross-validation counters and the fusion weights made from them at `tau`.  CustomCLIP.save_bank /
load_bank (ovmr_amd/modules.py) write and install it; this module owns the format, the model fingerprint and the checks of a file."""
from __future__ import annotations

import hashlib
import os
import os.path as osp
from typing import Dict, List, Optional

import numpy as np
import torch

BANK_FORMAT = 1
BANK_FILE = "reference_bank.pt"

# name -> (dtype, dimensions); C classes, R = sum(shots) exemplar rows, D = embed_dim, L = context_length
TENSORS = {
    "tokenized_prompts": (torch.int64, 2),       # [C, L]
    "shots": (torch.int32, 1),                   # [C]
    "features": (torch.float16, 2),              # [R, D]
    "mm_classifier": (torch.float16, 2),         # [C, D]
    "vision_classifier": (torch.float16, 2),     # [C, D]
    "text_classifier": (torch.float16, 2),       # [C, D]
    "visual_tokens": (torch.float16, 3),         # [C, n_ctx, D]
    "xval_counts": (torch.int32, 3),             # [3, 2, C]
    "fusion_weight": (torch.float32, 2),         # [C, 3]
}
FIELDS = ("format", "fingerprint", "n_ctx", "embed_dim", "tau", "num_shots_cap", "classnames", "exemplar_paths") + tuple(TENSORS)

# the CLIP tensors the fingerprint reads: both projections, logit_scale, ln_final, the two positional embeddings, and the vision tower's
# first layer (class embedding and patch convolution)
FINGERPRINT_CLIP_KEYS = ("visual.proj", "text_projection", "logit_scale", "ln_final.weight", "ln_final.bias", "positional_embedding",
                         "visual.positional_embedding", "visual.class_embedding", "visual.conv1.weight")


def _as_tensor(v) -> torch.Tensor:
    return torch.from_numpy(v) if isinstance(v, np.ndarray) else torch.as_tensor(v)


def fingerprint(spec, n_ctx: int, prompt_learner_state: Dict[str, torch.Tensor], clip_state: Dict[str, torch.Tensor]) -> str:
    """sha256 (hex) over the model spec's geometry, n_ctx, every tensor of the prompt learner's state (in key order) and the CLIP tensors
    of FINGERPRINT_CLIP_KEYS, each as its name, its shape and its values as fp32.  A FINGERPRINT, not a proof: it tells a bank written
    under another prompt-learner checkpoint or another CLIP checkpoint apart from this model's (two CLIP checkpoints that agree on every
    listed tensor and differ elsewhere are not told apart), so that an edit cannot silently mix rows of two models."""
    h = hashlib.sha256()
    geometry = [(k, v) for k, v in sorted(vars(spec).items()) if k != "name"]
    h.update(repr((geometry, int(n_ctx))).encode())
    for title, sd, keys in (("prompt_learner", prompt_learner_state, sorted(prompt_learner_state)), ("clip", clip_state, FINGERPRINT_CLIP_KEYS)):
        for k in keys:
            if k not in sd:
                raise KeyError(f"fingerprint: the {title} state holds no {k!r}")
            t = _as_tensor(sd[k]).detach().float().cpu().contiguous()
            h.update(f"{title}.{k}{tuple(t.shape)}".encode())
            h.update(t.numpy().tobytes())
    return h.hexdigest()


def write(path: str, bank: dict) -> None:
    """torch.save of `bank` under `path`, written under a scratch name next to it and moved into place whole (as the classifier files
    are): a reader never finds a half-written bank."""
    missing = [k for k in FIELDS if k not in bank]
    if missing:
        raise ValueError(f"a reference bank needs the fields {missing}")
    d = osp.dirname(osp.abspath(path))
    os.makedirs(d, exist_ok=True)
    scratch = osp.join(d, f".partial.{os.getpid()}.{osp.basename(path)}")
    try:
        torch.save({k: bank[k] for k in FIELDS}, scratch)
        os.replace(scratch, path)
    finally:
        if osp.exists(scratch):
            os.remove(scratch)


def _refuse(path: str, field: str, why: str):
    raise ValueError(f'"{path}": {field} {why}')


def read(path: str) -> dict:
    """Reads a bank with the restricted reader (checkpoint._torch_load: nothing in the file can run code) and checks the file in itself: a
    ValueError that names the file and the field for a file that is not a bank, a newer format, fields of the wrong type or of shapes that
    do not describe one vocabulary.  check_model holds it against a model."""
    from . import checkpoint
    obj = checkpoint._torch_load(path)
    if not isinstance(obj, dict) or not isinstance(obj.get("format"), int) or isinstance(obj.get("format"), bool):
        _refuse(path, "format", "is missing: not a reference bank (CustomCLIP.save_bank writes one)")
    if obj["format"] > BANK_FORMAT:
        _refuse(path, "format", f"is {obj['format']}, this build reads reference banks up to format {BANK_FORMAT}")
    for k in FIELDS:
        if k not in obj:
            _refuse(path, k, "is missing: not a reference bank")
    for k, (dtype, dim) in TENSORS.items():
        t = obj[k]
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != dim:
            _refuse(path, k, f"must be a {dtype} tensor of {dim} dimensions, got "
                    + (f"{t.dtype} {list(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__))
    for k in ("n_ctx", "embed_dim", "num_shots_cap"):
        if not isinstance(obj[k], int):
            _refuse(path, k, f"must be an integer, got {type(obj[k]).__name__}")
    if not isinstance(obj["tau"], (int, float)) or not isinstance(obj["fingerprint"], str):
        _refuse(path, "tau / fingerprint", "must be a number and a string")
    C, L = obj["tokenized_prompts"].shape
    D, nc = obj["embed_dim"], obj["n_ctx"]
    if C < 1:
        _refuse(path, "tokenized_prompts", "holds no class")
    shots = obj["shots"]
    if tuple(shots.shape) != (C,) or int(shots.min()) < 1:
        _refuse(path, "shots", f"must hold one count >= 1 for each of the {C} classes, got {list(shots.shape)}")
    R = int(shots.sum())
    want = {"features": (R, D), "mm_classifier": (C, D), "vision_classifier": (C, D), "text_classifier": (C, D),
            "visual_tokens": (C, nc, D), "xval_counts": (3, 2, C), "fusion_weight": (C, 3)}
    for k, shape in want.items():
        if tuple(obj[k].shape) != shape:
            _refuse(path, k, f"is {list(obj[k].shape)}, the bank's {C} classes, {R} exemplar rows and width {D} need {list(shape)}")
    for k, n in (("classnames", C), ("exemplar_paths", R)):
        v = obj[k]
        if v is not None and not (isinstance(v, (list, tuple)) and len(v) == n and all(isinstance(x, str) for x in v)):
            _refuse(path, k, f"must be None or a list of {n} strings")
    return obj


def check_model(path: str, obj: dict, n_ctx: int, embed_dim: int, context_length: int, model_fingerprint: str) -> None:
    """A bank (as `read` returned it) against the model that is to load it: another n_ctx, another width or context length, another
    fingerprint are ValueErrors that name the file and the field."""
    if obj["n_ctx"] != n_ctx:
        _refuse(path, "n_ctx", f"is {obj['n_ctx']}, this model has n_ctx {n_ctx}")
    if obj["embed_dim"] != embed_dim:
        _refuse(path, "embed_dim", f"is {obj['embed_dim']}, this model's width is {embed_dim}")
    if obj["tokenized_prompts"].shape[1] != context_length:
        _refuse(path, "tokenized_prompts", f"has context length {obj['tokenized_prompts'].shape[1]}, this model's is {context_length}")
    if obj["fingerprint"] != model_fingerprint:
        _refuse(path, "fingerprint", f"is {obj['fingerprint'][:12]}..., this model's is {model_fingerprint[:12]}...: the bank was written "
                "under another CLIP checkpoint or another prompt-learner checkpoint")


def first_difference(a: List[str], b: List[str]) -> Optional[str]:
    """One line that names the first difference between two class-name lists, or None when they are equal."""
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return f"class {i} is {x!r} in the bank and {y!r} in the data set"
    if len(a) != len(b):
        return f"the bank has {len(a)} classes, the data set {len(b)}"
    return None
