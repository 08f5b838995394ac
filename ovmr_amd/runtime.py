"""ctypes binding to libovmr_hip.so (include/ovmr_hip.h) -- orchestration only.

PyTorch is used for device memory and streams: every tensor handed to the library is a torch
CUDA(=HIP) tensor, the library receives `tensor.data_ptr()` and the current stream.  There is no
CPU fallback: constructing an Engine without the HIP library or without a GPU raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Optional

import numpy as np
import torch

from .synth import ModelSpec

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libovmr_hip.so")

F16, F32, I64, I32 = 0, 1, 2, 3
MODES = {"fusion": 0, "text": 1, "vision": 2, "multimodal": 3}
ALL_MODES = ("fusion", "text", "vision", "multimodal")          # EVAL_MODE all: the plane order of ovmr_fused_logits_all (plane = MODES value)

c_p = ctypes.c_void_p
c_i = ctypes.c_int


class ModelDesc(ctypes.Structure):
    _fields_ = [(n, c_i) for n in ("embed_dim", "image_resolution", "vision_layers", "vision_width",
                                   "vision_patch_size", "context_length", "vocab_size", "transformer_width",
                                   "transformer_layers", "n_ctx", "agg_layers")]


class ResizeJob(ctypes.Structure):
    """ovmr_resize_job (include/ovmr_hip.h)."""
    _fields_ = [("in_offset", ctypes.c_int64), ("tmp_offset", ctypes.c_int64), ("w", c_i), ("h", c_i), ("y0", c_i), ("ny", c_i),
                ("table", c_i), ("ksize_h", c_i), ("ksize_v", c_i), ("passthrough", c_i)]


class TextGroup(ctypes.Structure):
    """ovmr_text_group (include/ovmr_hip.h)."""
    _fields_ = [("prompts_f16", c_p), ("ids", c_p), ("index", c_p), ("n", c_i), ("seq_len", c_i), ("normalize", c_i), ("out_f16", c_p)]


# name -> (restype, argtypes); mirrors include/ovmr_hip.h one to one
SIGNATURES = {
    "ovmr_create": (c_i, [ctypes.POINTER(ModelDesc), ctypes.POINTER(c_p)]),
    "ovmr_destroy": (None, [c_p]),
    "ovmr_last_error": (ctypes.c_char_p, [c_p]),
    "ovmr_version": (ctypes.c_char_p, []),
    "ovmr_set_option": (c_i, [c_p, ctypes.c_char_p, c_i]),
    "ovmr_set_weight": (c_i, [c_p, ctypes.c_char_p, c_p, c_i, c_i, ctypes.POINTER(ctypes.c_int64), c_p]),
    "ovmr_finalize": (c_i, [c_p, c_i, c_i, c_i, c_p]),
    "ovmr_encode_image": (c_i, [c_p, c_p, c_i, c_i, c_p, c_i, c_p]),
    "ovmr_encode_text_embedded": (c_i, [c_p, c_p, c_p, c_i, c_i, c_p, c_i, c_p]),
    "ovmr_encode_text_ids": (c_i, [c_p, c_p, c_i, c_i, c_p, c_i, c_p]),
    "ovmr_encode_text_groups": (c_i, [c_p, ctypes.POINTER(TextGroup), c_i, c_p]),
    "ovmr_encode_text_ensemble": (c_i, [c_p, c_p, c_i, c_i, ctypes.POINTER(ctypes.c_int32), c_p, c_p]),
    "ovmr_embed_tokens": (c_i, [c_p, c_p, c_i, c_i, c_p, c_p]),
    "ovmr_generate_tokens": (c_i, [c_p, c_p, c_i, c_i, c_p, c_p]),
    "ovmr_generate_tokens_ragged": (c_i, [c_p, c_p, ctypes.POINTER(ctypes.c_int32), c_p, c_i, c_i, c_p, c_p]),
    "ovmr_assemble_prompts": (c_i, [c_p, c_p, c_p, c_p, c_i, c_p, c_p]),
    "ovmr_xval_counts": (c_i, [c_p, c_p, c_p, c_i, c_p, c_i, c_p, c_p, c_p]),
    "ovmr_fusion_weights": (c_i, [c_p, c_p, c_p, c_i, ctypes.c_float, c_p, c_p]),
    "ovmr_fused_logits": (c_i, [c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_p, c_p]),
    "ovmr_fused_logits_all": (c_i, [c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_i, c_p, ctypes.c_long, c_p]),
    "ovmr_pack_rows": (c_i, [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_p]),
    "ovmr_unpack_rows": (c_i, [c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p]),
    "ovmr_eval_counts": (c_i, [c_p, c_i, ctypes.c_long, c_p, c_i, c_i, c_p, c_p]),
    "ovmr_topk_rows": (c_i, [c_p, c_i, ctypes.c_long, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p]),
    "ovmr_eval_detail": (c_i, [c_p, c_i, ctypes.c_long, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p]),
    "ovmr_head_plan": (c_i, [c_p, c_i, c_i]),
    "ovmr_zeroshot_logits": (c_i, [c_p, c_p, c_i, c_p, c_i, c_p, c_p]),
    "ovmr_logit_scale": (ctypes.c_float, [c_p]),
    "ovmr_preprocess_u8": (c_i, [c_p, c_i, c_i, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), c_p, c_p]),
    "ovmr_resize_crop_u8": (c_i, [c_p, c_p, c_i, c_p, c_p, c_i, c_p, c_i, c_p]),
    "ovmr_encode_chunk": (ctypes.c_int, [c_p]),
    "ovmr_encode_plan": (c_i, [c_p, c_i, ctypes.POINTER(c_i), c_i]),
    "ovmr_flops_per_image": (ctypes.c_double, [c_p]),
    "ovmr_flops_per_image_executed": (ctypes.c_double, [c_p]),
    "ovmr_flops_executed": (ctypes.c_double, [c_p, c_i]),
    "ovmr_flops_per_prompt": (ctypes.c_double, [c_p, c_i]),
    "ovmr_debug_gemm": (c_i, [c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, ctypes.c_float, c_i, c_i, c_p]),
    "ovmr_debug_lnfold": (c_i, [c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_p]),
    "ovmr_debug_layernorm": (c_i, [c_i, c_p, c_p, c_p, c_p, c_i, c_i, ctypes.c_long, c_p]),
    "ovmr_debug_attention": (c_i, [c_i, c_i, c_p, c_p, c_i, c_i, c_i, c_i, c_p]),
    "ovmr_debug_l2norm": (c_i, [c_p, c_i, c_i, c_i, c_p]),
    "ovmr_debug_text_ensemble": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p]),
    "ovmr_debug_text_embed_ids": (c_i, [c_p, c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p]),
    "ovmr_debug_text_add_pos": (c_i, [c_p, c_i, c_p, c_p, c_i, c_i, c_i, c_p]),
    "ovmr_debug_gather_rows": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_p]),
    "ovmr_debug_im2col": (c_i, [c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_p]),
    "ovmr_debug_fill_cls": (c_i, [c_p, c_p, c_i, c_i, c_i, c_p]),
    "ovmr_debug_gemm_patches": (c_i, [c_i, c_p, c_i, c_p, c_p, c_p, c_i, c_i, c_p]),
    "ovmr_debug_gemm_strided": (c_i, [c_i, c_p, c_i, c_p, c_i, c_p, c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_i, ctypes.c_float, c_p, c_p,
                                      c_i, c_p]),
    "ovmr_debug_attention_f32_varlen": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p]),
    "ovmr_debug_attention_f32_long": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p]),
    "ovmr_debug_attention_q": (c_i, [c_i, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "ovmr_debug_attention_route": (c_i, [c_i, c_i, c_i, c_i]),
    "ovmr_debug_gemm_route": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, ctypes.POINTER(c_i)]),
    "ovmr_debug_gemm_tile_kernels": (c_i, [ctypes.POINTER(c_i), c_i]),
    "ovmr_debug_fill_workspace": (c_i, [c_p, ctypes.c_uint32, c_p]),
}

# the extension header include/ovmr_hip_nearest.h, mirrored the same way (tests/test_nearest_cpu.py holds the pair to each other)
EXT_SIGNATURES = {
    "ovmr_nearest_scratch_bytes": (ctypes.c_long, [c_i, ctypes.c_long, c_i]),
    "ovmr_nearest_rows": (c_i, [c_p, c_i, c_p, ctypes.c_long, c_i, c_i, c_p, c_p, c_p, c_p, ctypes.c_long, c_p]),
    "ovmr_debug_nearest_rows": (c_i, [c_p, c_i, c_p, ctypes.c_long, c_i, c_i, c_p, c_p, c_p, c_p, ctypes.c_long, c_i, c_p]),
}

# the second extension header include/ovmr_hip_audit.h (tests/test_audit_cpu.py holds the pair to each other)
AUDIT_SIGNATURES = {
    "ovmr_neighbours_scratch_bytes": (ctypes.c_long, [c_i, ctypes.c_long, c_i, c_i]),
    "ovmr_neighbours_rows": (c_i, [c_p, c_i, c_p, ctypes.c_long, c_i, c_i, c_p, c_p, c_i, c_p, c_p, c_p, ctypes.c_long, c_p]),
    "ovmr_debug_neighbours_rows": (c_i, [c_p, c_i, c_p, ctypes.c_long, c_i, c_i, c_p, c_p, c_i, c_p, c_p, c_p, ctypes.c_long, c_i, c_i, c_p]),
}

# the third extension header include/ovmr_hip_retrieve.h (tests/test_retrieve_cpu.py holds the pair to each other)
RETRIEVE_SIGNATURES = {
    "ovmr_retrieve_state_bytes": (ctypes.c_long, [c_i, c_i]),
    "ovmr_retrieve_reset": (c_i, [c_p, c_i, c_i, c_p]),
    "ovmr_retrieve_update": (c_i, [c_p, c_i, ctypes.c_long, c_i, c_i, c_i, ctypes.c_long, c_p, c_p, c_p]),
    "ovmr_retrieve_merge": (c_i, [c_p, c_p, c_i, c_i, c_p]),
    "ovmr_retrieve_finish": (c_i, [c_p, c_i, c_i, c_p, c_p, c_p]),
}

# the fourth extension header include/ovmr_hip_curves.h (tests/test_curves_cpu.py holds the pair to each other)
CURVES_SIGNATURES = {
    "ovmr_eval_curves_state_bytes": (ctypes.c_long, [c_i, c_i]),
    "ovmr_eval_curves": (c_i, [c_p, c_i, ctypes.c_long, c_p, c_i, c_i, ctypes.c_float, ctypes.c_float, c_i, c_p, c_p]),
}

# the fifth extension header include/ovmr_hip_ranks.h (tests/test_ranks_cpu.py holds the pair to each other)
RANKS_SIGNATURES = {
    "ovmr_eval_ranks_state_cells": (ctypes.c_long, [c_i, ctypes.c_long]),
    "ovmr_eval_ranks": (c_i, [c_p, c_i, ctypes.c_long, c_p, c_i, c_i, c_p, c_p, ctypes.c_long, c_i, c_p, c_p]),
}

# the sixth extension header include/ovmr_hip_probe.h (tests/test_probe_cpu.py holds the pair to each other)
PROBE_SIGNATURES = {
    "ovmr_probe_logits": (c_i, [c_p, ctypes.c_long, c_i, c_p, c_p, c_i, c_i, c_p, ctypes.c_long, c_p]),
    "ovmr_probe_row_quantum": (c_i, []),
    "ovmr_probe_workspace_bytes": (ctypes.c_long, [c_i, c_i, c_i]),
    "ovmr_probe_loss_grad": (c_i, [c_p, ctypes.c_long, c_p, c_i, c_i, c_i, c_p, c_p, ctypes.c_float, ctypes.c_float, c_i, c_p, c_p, c_p, c_p,
                                   c_p]),
}

_lib = None


def load_library(path: Optional[str] = None) -> ctypes.CDLL:
    """Load libovmr_hip.so and bind every symbol of the C ABI.  Raises if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("OVMR_HIP_LIB", LIB_PATH)
    if not os.path.exists(p):
        raise RuntimeError(f"{p} not found: build it with `python -m ovmr_amd.build` (hipcc, gfx950). "
                           "ovmr_amd has no CPU fallback.")
    lib = ctypes.CDLL(p)
    for name, (res, args) in (list(SIGNATURES.items()) + list(EXT_SIGNATURES.items()) + list(AUDIT_SIGNATURES.items())
                              + list(RETRIEVE_SIGNATURES.items()) + list(CURVES_SIGNATURES.items()) + list(RANKS_SIGNATURES.items())
                              + list(PROBE_SIGNATURES.items())):
        fn = getattr(lib, name)          # AttributeError if the .so does not export the symbol
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def _ptr(t: Optional[torch.Tensor]):
    """The ONE place a tensor becomes an address for the library (the struct fields of encode_text_groups included; loader.preprocess_u8
    and evaluator.Classification go through it too): tests/test_boundary_cpu.py patches it to learn which tensor stands behind an address."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream_on(dev):
    """The current stream of device `dev` (None: of the current device) as the library takes it; the wrappers outside Engine follow their
    operands' device."""
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _stream():
    return _stream_on(None)


class OvmrError(RuntimeError):
    pass


def _refuse(where: str, name: str, want: str, got: str):
    raise ValueError(f"{where}: {name} must be {want}, got {got}")


def _same_device(a: torch.device, b) -> bool:
    if isinstance(b, str) and ":" not in b:                       # "cuda": any GPU
        return a.type == b
    b = torch.device(b)
    return a.type == b.type and (a.index == b.index or a.index is None or b.index is None)


def _want(where: str, name: str, t, shape=None, dtype=None, device=None, dense: bool = False, at_least: Optional[int] = None):
    """The operand check of every wrapper, stated once: the library sees an address and a few integers, never a shape (include/ovmr_hip.h),
    so what the integers promise is compared with the tensor here, before anything is copied, allocated or enqueued.  Metadata only --
    shape, dtype, device, strides: no device memory is read and nothing synchronises.  shape: one entry per dimension, None = any extent;
    at_least: the fewest elements.  dtype (one or a tuple), device and dense are for operands the library takes as they are (outputs,
    accumulators, the evaluator's inputs); what Engine._dev repairs (host or numpy input, another dtype, a strided view) is left to it.
    Raises ValueError naming the wrapper, the argument, what it must be and what it is."""
    if not isinstance(t, (torch.Tensor, np.ndarray)):
        _refuse(where, name, "a torch.Tensor or a numpy array", type(t).__name__)
    got = tuple(t.shape)
    if shape is not None and (len(got) != len(shape) or any(w is not None and int(w) != g for w, g in zip(shape, got))):
        _refuse(where, name, "of shape [" + ", ".join("*" if w is None else str(int(w)) for w in shape) + "]", f"{list(got)}")
    if at_least is not None and int(np.prod(got, dtype=np.int64)) < at_least:
        _refuse(where, name, f"of at least {at_least} elements", f"{list(got)}")
    if dtype is None and device is None and not dense:
        return
    if not isinstance(t, torch.Tensor):
        _refuse(where, name, "a torch.Tensor (the library takes it as it is)", "a numpy array")
    if dtype is not None and t.dtype not in (dtype if isinstance(dtype, tuple) else (dtype,)):
        _refuse(where, name, " / ".join(str(d) for d in (dtype if isinstance(dtype, tuple) else (dtype,))), str(t.dtype))
    if device is not None and not _same_device(t.device, device):
        _refuse(where, name, f"on {device}", f"a tensor on {t.device}")
    if dense and not t.is_contiguous():
        _refuse(where, name, "contiguous", f"strides {tuple(t.stride())} for shape {list(got)}")


def _want_range(where: str, name: str, t, lo: int, hi: int, what: str):
    """Values are checked on HOST operands only (as the EOT checks below): a device tensor would need a read-back, and stays the caller's
    contract."""
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(t)
    if t.is_cuda or not t.numel() or t.is_floating_point():
        return
    mn, mx = (int(x) for x in torch.aminmax(t))
    if mn < lo or mx >= hi:
        _refuse(where, name, f"{what} in [{lo}, {hi})", f"values from {mn} to {mx}")


def _want_rows(where: str, name: str, mo):
    """outputs [B, C] of the evaluator's entry points: fp16 / fp32 on the GPU, taken as it is."""
    _want(where, name, mo, (None, None), (torch.float16, torch.float32), "cuda")


def _row_matrix(where: str, name: str, mo) -> int:
    """mo [B, C] as the library reads it without a copy: unit column stride, rows at least C elements apart -> ld, the row stride to
    hand over (a single row's stride says nothing: at least C)."""
    B, C = mo.shape
    if C > 1 and mo.stride(1) != 1 or B > 1 and mo.stride(0) < C:
        _refuse(where, name, f"rows of unit column stride, at least {C} elements apart", f"strides {tuple(mo.stride())}")
    return mo.stride(0) if B > 1 else max(C, mo.stride(0))


def _want_out_pair(where: str, out, shape, index_dtype, dev):
    """out = (values fp32, indices) of a selection: both of `shape`, dense, on dev; None = the wrapper allocates."""
    if out is None:
        return
    if not isinstance(out, (tuple, list)) or len(out) != 2:
        _refuse(where, "out", "a pair (values, indices)", type(out).__name__)
    _want(where, "out[0]", out[0], shape, torch.float32, dev, dense=True)
    _want(where, "out[1]", out[1], shape, index_dtype, dev, dense=True)


def topk_rows(mo: torch.Tensor, k: int, labels: Optional[torch.Tensor] = None, hits: Optional[torch.Tensor] = None):
    """ovmr_topk_rows on the current stream: mo [B, C] fp16 / fp32 on the GPU (rows may be strided: stride(1) == 1, stride(0) >= C, no
    copy) -> (values fp32 [B, k], indices int32 [B, k]), best first in the library's total order (include/ovmr_hip.h).  labels int64 [B]
    and hits int32 [1] (both on the GPU, together or not at all): hits[0] += rows whose label is among their k columns."""
    _want_rows("topk_rows", "mo", mo)
    B, C = mo.shape
    if (labels is None) != (hits is None):
        raise ValueError("topk_rows takes labels and hits together or not at all")
    if labels is not None:
        _want("topk_rows", "labels", labels, (B,), torch.int64, mo.device, dense=True)
        _want("topk_rows", "hits", hits, None, torch.int32, mo.device, at_least=1)
    lib = load_library()
    if B > 1 and mo.stride(1) == 1 and mo.stride(0) < C:
        mo = mo.contiguous()                         # (an expanded row: not a row view of a matrix)
    elif C > 1 and mo.stride(1) != 1:
        mo = mo.contiguous()
    with torch.cuda.device(mo.device):
        values = torch.empty((B, int(k)), dtype=torch.float32, device=mo.device)
        indices = torch.empty((B, int(k)), dtype=torch.int32, device=mo.device)
        ld = _row_matrix("topk_rows", "mo", mo)
        rc = lib.ovmr_topk_rows(_ptr(mo), F32 if mo.dtype == torch.float32 else F16, ld, B, C, int(k), _ptr(values), _ptr(indices),
                                _ptr(labels), _ptr(hits), _stream_on(mo.device))
    if rc != 0:
        raise OvmrError(f"ovmr_topk_rows failed with {rc} (B = {B}, C = {C}, k = {k})")
    return values, indices


def eval_detail(mo: torch.Tensor, labels: torch.Tensor, k: int, counts: torch.Tensor, hits: Optional[torch.Tensor] = None,
                class_hits: Optional[torch.Tensor] = None, cmat: Optional[torch.Tensor] = None):
    """ovmr_eval_detail on the current stream: mo [B, C] fp16 / fp32 on the GPU (stride(1) == 1, stride(0) >= C), labels int64 [B];
    counts int32 [3C + 1], hits int32 [1], class_hits int32 [C], cmat int32 [C, C] (the last three optional) accumulate
    (include/ovmr_hip.h)."""
    _want_rows("eval_detail", "mo", mo)
    B, C = mo.shape
    ld = _row_matrix("eval_detail", "mo", mo)
    _want("eval_detail", "labels", labels, (B,), torch.int64, mo.device, dense=True)
    if counts is None:
        raise ValueError("eval_detail needs counts")
    for name, t, n in (("counts", counts, 3 * C + 1), ("hits", hits, 1), ("class_hits", class_hits, C), ("cmat", cmat, C * C)):
        if t is not None:
            _want("eval_detail", name, t, None, torch.int32, mo.device, dense=True)
            if t.numel() != n:
                _refuse("eval_detail", name, f"of {n} elements", f"{list(t.shape)}")
    lib = load_library()
    with torch.cuda.device(mo.device):
        rc = lib.ovmr_eval_detail(_ptr(mo), F32 if mo.dtype == torch.float32 else F16, ld, _ptr(labels), B, C, int(k), _ptr(counts),
                                  _ptr(hits), _ptr(class_hits), _ptr(cmat), _stream_on(mo.device))
    if rc != 0:
        raise OvmrError(f"ovmr_eval_detail failed with {rc} (B = {B}, C = {C}, k = {k})")


MAX_BINS = 4096                                                   # ovmr_eval_curves: the ceiling of bins (include/ovmr_hip_curves.h)


def curve_scale(lo, hi, bins: int, where: str = "eval_curves"):
    """(lo, hi, scale) of the slot function of include/ovmr_hip_curves.h as numpy float32: lo and hi rounded to fp32, lo < hi, both finite,
    scale = fp32(bins) / (hi - lo) with the subtraction and the division rounded once each, finite and positive -- what the launcher
    computes on the host.  Raises ValueError otherwise."""
    for name, v in (("lo", lo), ("hi", hi)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            _refuse(where, name, "a number", type(v).__name__)
    with np.errstate(all="ignore"):
        flo, fhi = np.float32(lo), np.float32(hi)
        if not np.isfinite(flo) or not np.isfinite(fhi):
            _refuse(where, "lo" if not np.isfinite(flo) else "hi", "finite as fp32", repr(lo if not np.isfinite(flo) else hi))
        if not flo < fhi:
            _refuse(where, "hi", f"above lo = {float(flo)!r} as fp32", repr(hi))
        scale = np.float32(bins) / np.float32(fhi - flo)
    if not np.isfinite(scale) or not scale > 0:
        _refuse(where, "hi", f"far enough from lo for bins / (hi - lo) to be a finite positive fp32 (bins = {bins})", f"lo = {lo!r}, hi = {hi!r}")
    return flo, fhi, scale


def eval_curves(mo: torch.Tensor, labels: torch.Tensor, lo: float, hi: float, bins: int, state: torch.Tensor):
    """ovmr_eval_curves on the current stream (include/ovmr_hip_curves.h): mo [B, C] fp16 / fp32 on the GPU (stride(1) == 1, stride(0) >= C,
    no copy), labels int64 [B]; state int32 [C, 2, bins + 3] accumulates: for every row whose label lies in [0, C) and every class c,
    state[c, labels[b] == c, slot(mo[b, c])] += 1 with the slot function of the header over [lo, hi) in `bins` bins.  One launch; an empty
    batch launches nothing."""
    where = "eval_curves"
    _want_rows(where, "mo", mo)
    B, C = mo.shape
    if C < 1:
        _refuse(where, "mo", "of at least one column", f"{list(mo.shape)}")
    ld = _row_matrix(where, "mo", mo)
    _want(where, "labels", labels, (B,), torch.int64, mo.device, dense=True)
    bins = _want_int(where, "bins", bins, 1, MAX_BINS)
    flo, fhi, _ = curve_scale(lo, hi, bins, where)
    _want(where, "state", state, (C, 2, bins + 3), torch.int32, mo.device, dense=True)
    lib = load_library()
    if B == 0:
        return
    with torch.cuda.device(mo.device):
        rc = lib.ovmr_eval_curves(_ptr(mo), F32 if mo.dtype == torch.float32 else F16, ld, _ptr(labels), B, C, float(flo), float(fhi), bins,
                                  _ptr(state), _stream_on(mo.device))
    if rc != 0:
        raise OvmrError(f"ovmr_eval_curves failed with {rc} (B = {B}, C = {C}, lo = {float(flo)!r}, hi = {float(fhi)!r}, bins = {bins})")


def eval_ranks(mo: torch.Tensor, labels: torch.Tensor, edges: torch.Tensor, estart: torch.Tensor, state: torch.Tensor, max_edges: int):
    """ovmr_eval_ranks on the current stream (include/ovmr_hip_ranks.h): mo [B, C] fp16 / fp32 on the GPU (stride(1) == 1, stride(0) >= C,
    no copy), labels int64 [B]; edges fp32 [E] and estart int32 [C + 1] on the same device (class c owns edges[estart[c]:estart[c + 1]],
    its distinct positive scores, descending: evaluator.rank_edges); state int32 [2, 2E + C] accumulates: for every row whose label lies
    in [0, C) and every class c, state[labels[b] == c, 2 estart[c] + c + cell] += 1 with the cell rule of the header.  max_edges: the
    largest number of edges of one class, in [0, E].  One launch; an empty batch launches nothing."""
    where = "eval_ranks"
    _want_rows(where, "mo", mo)
    B, C = mo.shape
    if C < 1:
        _refuse(where, "mo", "of at least one column", f"{list(mo.shape)}")
    ld = _row_matrix(where, "mo", mo)
    _want(where, "labels", labels, (B,), torch.int64, mo.device, dense=True)
    _want(where, "edges", edges, (None,), torch.float32, mo.device, dense=True)
    E = edges.shape[0]
    _want(where, "estart", estart, (C + 1,), torch.int32, mo.device, dense=True)
    _want(where, "state", state, (2, 2 * E + C), torch.int32, mo.device, dense=True)
    max_edges = _want_int(where, "max_edges", max_edges, 0, E)
    lib = load_library()
    if B == 0:
        return
    with torch.cuda.device(mo.device):
        rc = lib.ovmr_eval_ranks(_ptr(mo), F32 if mo.dtype == torch.float32 else F16, ld, _ptr(labels), B, C, _ptr(edges) if E else None,
                                 _ptr(estart), E, max_edges, _ptr(state), _stream_on(mo.device))
    if rc != 0:
        raise OvmrError(f"ovmr_eval_ranks failed with {rc} (B = {B}, C = {C}, E = {E}, max_edges = {max_edges})")


PROBE_WORKSPACE_CAP = 1 << 30                                     # bytes of logits workspace probe_workspace allocates at most


def _want_probe(where: str, x, W, b):
    """The operands every probe entry point shares (include/ovmr_hip_probe.h): x fp32 [N, D] on the GPU, unit column stride, rows a
    multiple of 4 and at least D elements apart, 16-byte aligned; W fp32 [C, D] and b fp32 [C], dense, on x's device; D % 32 == 0.
    -> (N, C, D, ldx)."""
    _want(where, "x", x, (None, None), torch.float32, "cuda")
    N, D = x.shape
    if D < 32 or D % 32:
        _refuse(where, "x", "of a width D that is a positive multiple of 32", f"{list(x.shape)}")
    ldx = _row_matrix(where, "x", x)
    if ldx % 4:
        _refuse(where, "x", "rows a multiple of 4 elements apart", f"strides {tuple(x.stride())}")
    _want(where, "W", W, (None, D), torch.float32, x.device, dense=True)
    C = W.shape[0]
    if C < 1:
        _refuse(where, "W", "of at least one row", f"{list(W.shape)}")
    _want(where, "b", b, (C,), torch.float32, x.device, dense=True)
    for name, t in (("x", x), ("W", W)):
        if t.data_ptr() % 16:
            _refuse(where, name, "16-byte aligned", f"an address ending in {t.data_ptr() % 16:#x}")
    return N, C, D, ldx


def probe_logits(x: torch.Tensor, W: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ovmr_probe_logits on the current stream (include/ovmr_hip_probe.h): x fp32 [B, D] (stride(1) == 1, stride(0) >= D and a multiple
    of 4, no copy), W fp32 [C, D], b fp32 [C] -> out fp32 [B, C] = x W^T + b, the library's fp32 GEMM with its bias epilogue.  out: the
    caller's [B, C] (rows at least C apart: a column slice of a wider buffer is written in place and the rest left alone)."""
    where = "probe_logits"
    B, C, D, ldx = _want_probe(where, x, W, b)
    if out is not None:
        _want(where, "out", out, (B, C), torch.float32, x.device)
        ldo = _row_matrix(where, "out", out)
    lib = load_library()
    with torch.cuda.device(x.device):
        if out is None:
            out, ldo = torch.empty((B, C), dtype=torch.float32, device=x.device), C
        if B == 0:
            return out
        rc = lib.ovmr_probe_logits(_ptr(x), ldx, B, _ptr(W), _ptr(b), C, D, _ptr(out), ldo, _stream_on(x.device))
    if rc != 0:
        raise OvmrError(f"ovmr_probe_logits failed with {rc} (B = {B}, C = {C}, D = {D})")
    return out


def probe_rows_per_call(N: int, C: int, D: int, max_bytes: int = PROBE_WORKSPACE_CAP) -> int:
    """Rows one ovmr_probe_loss_grad call takes so that its logits stay within max_bytes: N where they fit, else the largest multiple of
    the library's row quantum that does (at least one quantum)."""
    lib = load_library()
    N, C, D = _want_int("probe_workspace", "N", N, 0, 2 ** 31 - 1), _want_int("probe_workspace", "C", C, 1, 2 ** 31 - 4), int(D)
    if lib.ovmr_probe_workspace_bytes(0, C, D) < 0:
        _refuse("probe_workspace", "D", "a positive multiple of 32", repr(D))
    q = lib.ovmr_probe_row_quantum()
    per_row = lib.ovmr_probe_workspace_bytes(1, C, D)
    return N if N * per_row <= max_bytes else max(q, int(max_bytes) // (per_row * q) * q)


def probe_workspace(N: int, C: int, D: int, device, max_bytes: int = PROBE_WORKSPACE_CAP) -> torch.Tensor:
    """The fp32 workspace of probe_loss_grad for N rows, at most max_bytes of it (or one row quantum's worth, if that is more): where
    the logits of all rows would take more, probe_loss_grad walks the rows in cuts that fit."""
    rows = probe_rows_per_call(N, C, D, max_bytes)
    nbytes = load_library().ovmr_probe_workspace_bytes(rows, C, D)
    with torch.cuda.device(device):
        return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


def probe_loss_grad(x: torch.Tensor, labels: torch.Tensor, W: torch.Tensor, b: torch.Tensor, inv_n: float, l2: float,
                    workspace: Optional[torch.Tensor] = None, gW: Optional[torch.Tensor] = None, gb: Optional[torch.Tensor] = None,
                    row_loss: Optional[torch.Tensor] = None):
    """ovmr_probe_loss_grad on the current stream (include/ovmr_hip_probe.h): the objective
    f = inv_n * sum_n (lse(z_n) - z_n[y_n]) + l2 / 2 * ||W||^2, z = x W^T + b, over x fp32 [N, D] and labels int64 [N] (a label outside
    [0, C) leaves its row out) -> (loss, gW, gb, row_loss): loss a 0-dim fp64 tensor on the device (row_loss summed in fp64, nothing is
    read back), gW fp32 [C, D] and gb fp32 [C] the gradient, row_loss fp32 [N] the per-row terms.  workspace: fp32, dense, from
    probe_workspace; where it holds fewer than N rows of logits the rows are walked in cuts that are multiples of the library's row
    quantum, the later ones with accumulate = 1 -- bit for bit the one-call result (the header says why)."""
    where = "probe_loss_grad"
    N, C, D, ldx = _want_probe(where, x, W, b)
    _want(where, "labels", labels, (N,), torch.int64, x.device, dense=True)
    for name, v in (("inv_n", inv_n), ("l2", l2)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0:
            _refuse(where, name, "a finite number, not negative", repr(v))
    lib = load_library()
    q = lib.ovmr_probe_row_quantum()
    per_row = lib.ovmr_probe_workspace_bytes(1, C, D) // 4
    if workspace is not None:
        _want(where, "workspace", workspace, (None,), torch.float32, x.device, dense=True)
        rows = N if workspace.numel() >= N * per_row else workspace.numel() // (per_row * q) * q
        if rows == 0 and N > 0:
            _refuse(where, "workspace", f"of at least {min(N, q) * per_row} elements (the logits of {min(N, q)} rows of {C} classes)",
                    f"{list(workspace.shape)}")
        if workspace.data_ptr() % 16:
            _refuse(where, "workspace", "16-byte aligned", f"an address ending in {workspace.data_ptr() % 16:#x}")
    for name, t, shape in (("gW", gW, (C, D)), ("gb", gb, (C,)), ("row_loss", row_loss, (N,))):
        if t is not None:
            _want(where, name, t, shape, torch.float32, x.device, dense=True)
    if gW is not None and gW.data_ptr() % 16:
        _refuse(where, "gW", "16-byte aligned", f"an address ending in {gW.data_ptr() % 16:#x}")
    with torch.cuda.device(x.device):
        if workspace is None:
            workspace = probe_workspace(N, C, D, x.device)
            rows = N if workspace.numel() >= N * per_row else workspace.numel() // (per_row * q) * q
        gW = torch.empty((C, D), dtype=torch.float32, device=x.device) if gW is None else gW
        gb = torch.empty((C,), dtype=torch.float32, device=x.device) if gb is None else gb
        row_loss = torch.empty((N,), dtype=torch.float32, device=x.device) if row_loss is None else row_loss
        stream = _stream_on(x.device)
        for n0 in range(0, max(N, 1), max(rows, 1)):
            n = min(rows, N - n0)
            rc = lib.ovmr_probe_loss_grad(_ptr(x[n0:]) if n else None, ldx, _ptr(labels[n0:]) if n else None, n, C, D, _ptr(W), _ptr(b),
                                          float(inv_n), float(l2), int(n0 > 0), _ptr(workspace) if n else None,
                                          _ptr(row_loss[n0:]) if n else None, _ptr(gW), _ptr(gb), stream)
            if rc != 0:
                raise OvmrError(f"ovmr_probe_loss_grad failed with {rc} (rows {n0} .. {n0 + n} of {N}, C = {C}, D = {D})")
        loss = row_loss.sum(dtype=torch.float64) * float(inv_n) + W.double().square().sum() * (0.5 * float(l2))
    return loss, gW, gb, row_loss


_nearest_scratch: Dict[torch.device, torch.Tensor] = {}       # per device: the scratch of nearest_rows, grown on demand


def _search_scratch(dev, need: int) -> torch.Tensor:
    """The cached scratch of device dev (the current device, inside the caller's torch.cuda.device), grown to `need` bytes."""
    key = torch.device(dev.type, torch.cuda.current_device())
    scratch = _nearest_scratch.get(key)
    if scratch is None or scratch.numel() * 8 < need:
        scratch = _nearest_scratch[key] = torch.empty(((need + 7) // 8,), dtype=torch.int64, device=dev)
    return scratch


def _want_search(where: str, queries, bank, k, out):
    """The operands nearest_rows and neighbour_rows share: queries [B, D] and bank [R, D], fp16 on one GPU, D a multiple of 64 in
    [64, 1024], 1 <= k <= min(R, 32), out None or a pair ([B, k] fp32, [B, k] int32) -> (B, D, R, k)."""
    _want(where, "queries", queries, (None, None), torch.float16, "cuda")
    _want(where, "bank", bank, (None, None), torch.float16, queries.device)
    B, D = queries.shape
    R = bank.shape[0]
    if bank.shape[1] != D:
        _refuse(where, "bank", f"of shape [*, {D}] (the queries' width)", f"{list(bank.shape)}")
    if D % 64 or not 64 <= D <= 1024:
        _refuse(where, "queries", "of a width that is a multiple of 64 in [64, 1024]", f"{list(queries.shape)}")
    k = _want_int(where, "k", k, 1, min(R, 32))
    _want_out_pair(where, out, (B, k), torch.int32, queries.device)
    return B, D, R, k


def nearest_rows(queries: torch.Tensor, bank: torch.Tensor, k: int, ranges: Optional[torch.Tensor] = None, out=None):
    """ovmr_nearest_rows on the current stream (include/ovmr_hip_nearest.h): queries [B, D] and bank [R, D], fp16 on the GPU, D a multiple of
    64 in [64, 1024], 1 <= k <= min(R, 32) -> (values fp32 [B, k], indices int32 [B, k]): per query the k bank rows of largest
    h(queries[b] . bank[r]), best first in the library's total order, equal scores to the lower row.  ranges int32 [B, 2] (lo, hi): query b
    looks at the rows lo <= r < hi only; fewer than k of them leave a tail of index -1, value -inf.  Host ranges are checked
    (0 <= lo <= hi <= R) and copied; device ranges are the caller's contract (the kernel clamps what it reads).  A strided queries / bank /
    ranges view is made contiguous.  out: (values, indices) to write into.  The scratch is one cached buffer per device: calls are
    ordered on one stream, like everything that shares a workspace."""
    where = "nearest_rows"
    B, D, R, k = _want_search(where, queries, bank, k, out)
    if ranges is not None:
        ranges = _want_pairs(where, "ranges", ranges, B, R, queries.device)
    lib = load_library()
    dev = queries.device
    with torch.cuda.device(dev):
        queries, bank = queries.contiguous(), bank.contiguous()
        if ranges is not None:
            ranges = ranges.to(dev, torch.int32).contiguous()
        values, indices = out if out is not None else (torch.empty((B, k), dtype=torch.float32, device=dev),
                                                        torch.empty((B, k), dtype=torch.int32, device=dev))
        if B == 0:
            return values, indices
        need = int(lib.ovmr_nearest_scratch_bytes(B, R, k))
        if need < 0:
            raise OvmrError(f"ovmr_nearest_scratch_bytes refuses B = {B}, R = {R}, k = {k}")
        scratch = _search_scratch(dev, need)
        rc = lib.ovmr_nearest_rows(_ptr(queries), B, _ptr(bank), R, D, k, _ptr(ranges), _ptr(values), _ptr(indices), _ptr(scratch),
                                   scratch.numel() * 8, _stream_on(dev))
    if rc != 0:
        raise OvmrError(f"ovmr_nearest_rows failed with {rc} (B = {B}, R = {R}, D = {D}, k = {k})")
    return values, indices


MAX_RANGE = 4096                                                  # ovmr_neighbours_rows: the ceiling of max_range (include/ovmr_hip_audit.h)


def _want_pairs(where: str, name: str, t, B: int, R: int, dev):
    """ranges of nearest_rows, ranges / exclude of neighbour_rows: [B, 2] of an integer dtype; host values are checked
    (0 <= lo <= hi <= R), device values are the caller's contract (the kernels clamp what they read).  Returns the tensor (a numpy array
    as a tensor)."""
    _want(where, name, t, (B, 2))
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(t)
    if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        _refuse(where, name, "of an integer dtype", str(t.dtype))
    if not t.is_cuda:
        _want_range(where, name, t, 0, R + 1, "row bounds")
        if t.numel() and bool((t[:, 0] > t[:, 1]).any()):
            _refuse(where, name, "pairs lo <= hi", "a pair with lo > hi")
    elif not _same_device(t.device, dev):
        _refuse(where, name, f"on {dev} or on the host", f"a tensor on {t.device}")
    return t


def neighbour_rows(queries: torch.Tensor, bank: torch.Tensor, k: int, ranges: Optional[torch.Tensor] = None,
                   exclude: Optional[torch.Tensor] = None, max_range: int = 0, out=None):
    """ovmr_neighbours_rows on the current stream (include/ovmr_hip_audit.h): nearest_rows with an excluded row range per query and a launch
    for short ranges.  queries [B, D], bank [R, D], k, ranges, out: as nearest_rows.  exclude int32 [B, 2] (xlo, xhi): query b leaves the
    rows xlo <= r < xhi out; host values are checked like ranges and copied, device values are clamped by the kernel.  max_range 0: the
    tiled launch pair; 1 .. 4096: a promise that no range is longer, which takes the one-wave-per-query launch (ranges required; host
    ranges are held to the promise, device ranges are truncated to it by the kernel).  The scratch is nearest_rows' cached buffer."""
    where = "neighbour_rows"
    B, D, R, k = _want_search(where, queries, bank, k, out)
    max_range = _want_int(where, "max_range", max_range, 0, MAX_RANGE)
    if max_range > 0 and ranges is None:
        _refuse(where, "ranges", f"given where max_range = {max_range} promises their length", "None")
    if ranges is not None:
        ranges = _want_pairs(where, "ranges", ranges, B, R, queries.device)
        if max_range > 0 and not ranges.is_cuda and ranges.numel() and int((ranges[:, 1] - ranges[:, 0]).max()) > max_range:
            _refuse(where, "ranges", f"pairs with hi - lo <= max_range = {max_range}", f"a range of {int((ranges[:, 1] - ranges[:, 0]).max())} rows")
    if exclude is not None:
        exclude = _want_pairs(where, "exclude", exclude, B, R, queries.device)
    lib = load_library()
    dev = queries.device
    with torch.cuda.device(dev):
        queries, bank = queries.contiguous(), bank.contiguous()
        if ranges is not None:
            ranges = ranges.to(dev, torch.int32).contiguous()
        if exclude is not None:
            exclude = exclude.to(dev, torch.int32).contiguous()
        values, indices = out if out is not None else (torch.empty((B, k), dtype=torch.float32, device=dev),
                                                        torch.empty((B, k), dtype=torch.int32, device=dev))
        if B == 0:
            return values, indices
        need = int(lib.ovmr_neighbours_scratch_bytes(B, R, k, max_range))
        if need < 0:
            raise OvmrError(f"ovmr_neighbours_scratch_bytes refuses B = {B}, R = {R}, k = {k}, max_range = {max_range}")
        scratch = _search_scratch(dev, need) if need else None
        rc = lib.ovmr_neighbours_rows(_ptr(queries), B, _ptr(bank), R, D, k, _ptr(ranges), _ptr(exclude), max_range, _ptr(values),
                                      _ptr(indices), _ptr(scratch), 0 if scratch is None else scratch.numel() * 8, _stream_on(dev))
    if rc != 0:
        raise OvmrError(f"ovmr_neighbours_rows failed with {rc} (B = {B}, R = {R}, D = {D}, k = {k}, max_range = {max_range})")
    return values, indices


MAX_PER_CLASS = 32                                                # ovmr_retrieve_*: the ceiling of m (include/ovmr_hip_retrieve.h)
MAX_POOL = 2 ** 32 - 1                                            # image indices lie in [0, MAX_POOL)


def _want_int(where: str, name: str, v, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        _refuse(where, name, f"an integer in [{lo}, {hi}]", repr(v))
    return int(v)


class ColumnTopM:
    """The m best images of each of C classes over a stream of [B, C] output matrices (include/ovmr_hip_retrieve.h): owns the state and
    calls ovmr_retrieve_update / _merge / _finish on the current stream.  The order is the library's total order on (score, image index):
    larger score first, equal scores to the lower image, NaN largest, -0 == +0.  `state` is the int64 [C, m] tensor itself -- opaque,
    all-zero = empty, byte-copyable: it goes through an all-gather as it is, and what comes back goes into merge().  The state is a
    function of what was offered, not of the batches it came in or of their order.  base is a scalar, so an update is for eager streams
    (a captured graph would replay the same base)."""

    def __init__(self, C: int, m: int, device="cuda:0"):
        self.C = _want_int("ColumnTopM", "C", C, 1, 2 ** 31 - 1)
        self.m = _want_int("ColumnTopM", "m", m, 1, MAX_PER_CLASS)
        self.device = torch.device(device)
        self.state = torch.zeros((self.C, self.m), dtype=torch.int64, device=self.device)

    def reset(self):
        """Empties every list (ovmr_retrieve_reset)."""
        with torch.cuda.device(self.device):
            rc = load_library().ovmr_retrieve_reset(_ptr(self.state), self.C, self.m, _stream_on(self.device))
        if rc != 0:
            raise OvmrError(f"ovmr_retrieve_reset failed with {rc} (C = {self.C}, m = {self.m})")
        return self

    def update(self, out: torch.Tensor, base: int, floor: Optional[torch.Tensor] = None):
        """Offers a batch: out [B, C] fp16 / fp32 on the state's device, taken as it is (rows may be strided: stride(1) == 1,
        stride(0) >= C); row b is image base + b of the pool, 0 <= base, base + B <= 2^32 - 1.  floor fp32 [B] (dense, same device):
        element (b, c) is offered only if it is not below floor[b] in the value order (equal is eligible; a NaN floor admits only NaNs)."""
        where = "ColumnTopM.update"
        _want_rows(where, "out", out)
        _want(where, "out", out, (None, self.C), device=self.device)
        B, C = out.shape
        ld = _row_matrix(where, "out", out)
        base = _want_int(where, "base", base, 0, MAX_POOL - B)
        if floor is not None:
            _want(where, "floor", floor, (B,), torch.float32, self.device, dense=True)
        if B == 0:
            return self
        lib = load_library()
        with torch.cuda.device(self.device):
            rc = lib.ovmr_retrieve_update(_ptr(out), F32 if out.dtype == torch.float32 else F16, ld, B, C, self.m, base, _ptr(floor),
                                          _ptr(self.state), _stream_on(self.device))
        if rc != 0:
            raise OvmrError(f"ovmr_retrieve_update failed with {rc} (B = {B}, C = {C}, m = {self.m}, base = {base})")
        return self

    def merge(self, other):
        """The state becomes that of both streams together (ovmr_retrieve_merge); they must hold disjoint images.  other: a ColumnTopM
        of the same C and m, or a state tensor int64 [C, m] (dense, same device), e.g. a rank's slice of an all-gather."""
        where = "ColumnTopM.merge"
        if isinstance(other, ColumnTopM):
            other = other.state
        _want(where, "other", other, (self.C, self.m), torch.int64, self.device, dense=True)
        if other.data_ptr() == self.state.data_ptr():
            _refuse(where, "other", "the state of ANOTHER stream (disjoint images)", "this object's own state")
        with torch.cuda.device(self.device):
            rc = load_library().ovmr_retrieve_merge(_ptr(self.state), _ptr(other), self.C, self.m, _stream_on(self.device))
        if rc != 0:
            raise OvmrError(f"ovmr_retrieve_merge failed with {rc} (C = {self.C}, m = {self.m})")
        return self

    def finish(self, out=None):
        """(values fp32 [C, m], indices int64 [C, m]) on the device, best first; an unfilled rank is index -1, value -inf.  The state
        stays as it is.  out: (values, indices) to write into."""
        where = "ColumnTopM.finish"
        _want_out_pair(where, out, (self.C, self.m), torch.int64, self.device)
        lib = load_library()
        with torch.cuda.device(self.device):
            values, indices = out if out is not None else (torch.empty((self.C, self.m), dtype=torch.float32, device=self.device),
                                                            torch.empty((self.C, self.m), dtype=torch.int64, device=self.device))
            rc = lib.ovmr_retrieve_finish(_ptr(self.state), self.C, self.m, _ptr(values), _ptr(indices), _stream_on(self.device))
        if rc != 0:
            raise OvmrError(f"ovmr_retrieve_finish failed with {rc} (C = {self.C}, m = {self.m})")
        return values, indices


class Engine:
    """One handle = one model on one device, used from one stream at a time."""

    def __init__(self, spec: ModelSpec, n_ctx: int = 2, device: str = "cuda:0"):
        if not torch.cuda.is_available():
            raise RuntimeError("ovmr_amd needs a ROCm GPU (MI355X / gfx950); there is no CPU fallback")
        self.lib = load_library()
        self.spec = spec
        self.n_ctx = n_ctx
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        desc = ModelDesc(spec.embed_dim, spec.image_resolution, spec.vision_layers, spec.vision_width,
                         spec.vision_patch_size, spec.context_length, spec.vocab_size, spec.transformer_width,
                         spec.transformer_layers, n_ctx, spec.agg_layers)
        h = c_p()
        rc = self.lib.ovmr_create(ctypes.byref(desc), ctypes.byref(h))
        if rc != 0:
            raise OvmrError(f"ovmr_create failed with {rc}")
        self.h = h
        self.finalized = False
        self._options: Dict[str, int] = {}       # what set_option was called with (a twin handle mirrors them: modules.CustomCLIP.forward_batches)
        self._weights_version = 0                # bumped by every set_weight

    def __del__(self):
        try:
            if getattr(self, "h", None):
                torch.cuda.synchronize(self.device)
                self.lib.ovmr_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _ck(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.ovmr_last_error(self.h)
            raise OvmrError(f"{what} failed with {rc}: {msg.decode() if msg else ''}")

    def _dev(self, t, dtype=None) -> torch.Tensor:
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(t)
        t = t.to(self.device, non_blocking=True)
        if dtype is not None and t.dtype != dtype:
            t = t.to(dtype)
        return t.contiguous()

    def set_option(self, key: str, value: int):
        self._ck(self.lib.ovmr_set_option(self.h, key.encode(), int(value)), "ovmr_set_option")
        self._options[key] = int(value)

    # ------------------------------------------------------------------ weights
    def set_weight(self, name: str, tensor):
        """tensor: a real-valued torch.Tensor or numpy array of the weight's own shape (fp16 and fp32 go as they are, anything else as fp32)."""
        _want(f"set_weight({name})", "tensor", tensor)
        if (torch.from_numpy(tensor) if isinstance(tensor, np.ndarray) else tensor).is_complex():
            _refuse(f"set_weight({name})", "tensor", "real-valued", str(tensor.dtype))
        t = self._dev(tensor)
        if t.dtype not in (torch.float16, torch.float32):
            t = t.float()
        shape = (ctypes.c_int64 * max(1, t.dim()))(*t.shape)
        rc = self.lib.ovmr_set_weight(self.h, name.encode(), _ptr(t), F16 if t.dtype == torch.float16 else F32,
                                      t.dim(), shape, _stream())
        self._ck(rc, f"ovmr_set_weight({name})")
        torch.cuda.current_stream().synchronize()   # the source tensor may be freed by the caller right after
        self.finalized = False
        self._weights_version += 1

    def load_state_dict(self, clip_sd: Dict[str, "torch.Tensor"], prompt_learner_sd: Optional[Dict] = None):
        """clip_sd: reference CLIP state dict (clip/model.py:899-936 key names); prompt_learner_sd:
        PromptLearner.state_dict() (trainers/mm_classifier_one_prompt.py:461-493)."""
        skip = ("input_resolution", "context_length", "vocab_size")    # clip/model.py:930-932
        for k, v in clip_sd.items():
            if k not in skip:
                self.set_weight(k, v)
        if prompt_learner_sd is not None:
            for k, v in prompt_learner_sd.items():
                if k in ("token_prefix", "token_suffix"):               # :482-487
                    continue
                self.set_weight("prompt_learner." + k, v)

    def finalize(self, max_images: int = 256, max_prompts: int = 256, max_classes: int = 1024):
        self._ck(self.lib.ovmr_finalize(self.h, max_images, max_prompts, max_classes, _stream()), "ovmr_finalize")
        self.finalized = True

    @property
    def logit_scale(self) -> float:
        return float(self.lib.ovmr_logit_scale(self.h))

    @property
    def encode_chunk(self) -> int:
        """Images per launch sequence of encode_image (chosen by ovmr_finalize so that the GEMM grids are whole rounds of the CUs)."""
        return int(self.lib.ovmr_encode_chunk(self.h))

    def encode_plan(self, B: int) -> list:
        """Image counts of the launch sequences encode_image runs a batch of B images as."""
        buf = (c_i * 4096)()
        n = int(self.lib.ovmr_encode_plan(self.h, int(B), buf, 4096))
        if n < 0:
            raise OvmrError("ovmr_encode_plan: the engine is not finalized")
        return [int(buf[i]) for i in range(min(n, 4096))]

    def flops_per_image(self) -> float:
        return float(self.lib.ovmr_flops_per_image(self.h))

    def flops_per_image_executed(self) -> float:
        return float(self.lib.ovmr_flops_per_image_executed(self.h))

    def flops_executed(self, B: int) -> float:
        """FLOPs ONE encode_image call on B images launches (the plan actually run, the 256-image Q rule per launch sequence)."""
        return float(self.lib.ovmr_flops_executed(self.h, int(B)))

    def flops_per_prompt(self, seq_len: int) -> float:
        return float(self.lib.ovmr_flops_per_prompt(self.h, seq_len))

    # ------------------------------------------------------------------ compute
    # Every wrapper below checks its operands against the handle's geometry FIRST (_want: shapes, and dtype / device / strides of what the
    # library takes as it is), then repairs layouts (_dev), allocates and launches: a refused call has copied and enqueued nothing.
    def check_image(self, image, where: str = "encode_image"):
        """image must be [B, 3, R, R] with R = spec.image_resolution (any dtype or layout; numpy and host tensors too).  For callers that
        slice or stage a batch before they encode it (modules._TwoInFlight, CustomCLIP._forward_split)."""
        R = self.spec.image_resolution
        _want(where, "image", image, (None, 3, R, R))

    def _want_ids(self, where: str, name: str, ids, shape):
        _want(where, name, ids, shape)
        _want_range(where, name, ids, 0, self.spec.vocab_size, "token ids")

    def encode_image(self, image: torch.Tensor, normalize: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """image [B, 3, R, R] (fp16 / fp32 go as they are, any other dtype as fp32) -> [B, embed_dim] fp16; out, when given: that tensor,
        fp16, contiguous, on the engine's device."""
        self.check_image(image)
        B = int(image.shape[0])
        if out is not None:
            _want("encode_image", "out", out, (B, self.spec.embed_dim), torch.float16, self.device, dense=True)
        image = self._dev(image)
        if image.dtype not in (torch.float16, torch.float32):
            image = image.float()
        if out is None:
            out = torch.empty((B, self.spec.embed_dim), dtype=torch.float16, device=self.device)
        self._ck(self.lib.ovmr_encode_image(self.h, _ptr(image), F16 if image.dtype == torch.float16 else F32, B,
                                            _ptr(out), int(normalize), _stream()), "ovmr_encode_image")
        return out

    def _want_prompts(self, where: str, prompts, index):
        sp = self.spec
        _want(where, "prompts", prompts, (None, sp.context_length, sp.transformer_width))
        _want(where, "index", index, (prompts.shape[0],))

    def encode_text_embedded(self, prompts: torch.Tensor, index: torch.Tensor, seq_len: Optional[int] = None,
                             normalize: int = 0) -> torch.Tensor:
        """prompts [N, context_length, transformer_width], index [N] (the read-out rows) -> [N, embed_dim] fp16."""
        self._want_prompts("encode_text_embedded", prompts, index)
        sl_req = int(seq_len) if seq_len is not None else self.spec.context_length
        if isinstance(index, torch.Tensor) and not index.is_cuda and index.numel() and int(index.max()) >= sl_req:
            raise ValueError(f"seq_len {sl_req} does not reach the largest read-out index {int(index.max())}")
        prompts = self._dev(prompts, torch.float16)
        index = self._dev(index, torch.int32)
        N = prompts.shape[0]
        out = torch.empty((N, self.spec.embed_dim), dtype=torch.float16, device=self.device)
        sl = int(seq_len) if seq_len is not None else self.spec.context_length
        self._ck(self.lib.ovmr_encode_text_embedded(self.h, _ptr(prompts), _ptr(index), N, sl, _ptr(out),
                                                    int(normalize), _stream()), "ovmr_encode_text_embedded")
        return out

    def encode_text_ids(self, ids: torch.Tensor, seq_len: Optional[int] = None, normalize: int = 0) -> torch.Tensor:
        """ids [N, context_length] (any integer dtype; host ids are held to [0, vocab_size)) -> [N, embed_dim] fp16."""
        self._want_ids("encode_text_ids", "ids", ids, (None, self.spec.context_length))
        if seq_len is not None and isinstance(ids, torch.Tensor) and not ids.is_cuda and ids.numel():
            eot = int(ids.argmax(dim=-1).max())                 # EOT has the largest id (clip/model.py:831)
            if eot >= int(seq_len):
                raise ValueError(f"seq_len {int(seq_len)} does not reach the EOT token at position {eot}")
        ids = self._dev(ids, torch.int64)
        N = ids.shape[0]
        out = torch.empty((N, self.spec.embed_dim), dtype=torch.float16, device=self.device)
        sl = int(seq_len) if seq_len is not None else self.spec.context_length
        self._ck(self.lib.ovmr_encode_text_ids(self.h, _ptr(ids), N, sl, _ptr(out), int(normalize), _stream()),
                 "ovmr_encode_text_ids")
        return out

    def encode_text_groups(self, groups) -> list:
        """Several prompt families in ONE pass of the text tower (ovmr_encode_text_groups).  Each group is a dict with either
        `prompts` [N, context_length, W] + `index` [N] or `ids` [N, context_length], and `seq_len`, `normalize` as the
        single-group calls.  Returns one [N, embed_dim] fp16 tensor per group."""
        for k, g in enumerate(groups):                       # every group is checked before the first one is copied
            where = f"encode_text_groups (group {k})"
            if g.get("ids") is not None:
                self._want_ids(where, "ids", g["ids"], (None, self.spec.context_length))
            else:
                self._want_prompts(where, g.get("prompts"), g.get("index"))
        arr = (TextGroup * len(groups))()
        keep, outs = [], []
        for a, g in zip(arr, groups):
            sl = int(g.get("seq_len") or self.spec.context_length)
            # the same host-side checks as the single-family calls (only for tensors that are on the host: no device read-back here)
            src = g.get("ids") if g.get("ids") is not None else g.get("index")
            if isinstance(src, torch.Tensor) and not src.is_cuda and src.numel():
                last = int(src.argmax(dim=-1).max()) if g.get("ids") is not None else int(src.max())
                if last >= sl:
                    raise ValueError(f"seq_len {sl} does not reach the read-out row {last} of a prompt group")
            if g.get("ids") is not None:
                ids = self._dev(g["ids"], torch.int64)
                keep.append(ids)
                a.prompts_f16, a.ids, a.index, n = None, _ptr(ids).value, None, ids.shape[0]
            else:
                pr, ix = self._dev(g["prompts"], torch.float16), self._dev(g["index"], torch.int32)
                keep += [pr, ix]
                a.prompts_f16, a.ids, a.index, n = _ptr(pr).value, None, _ptr(ix).value, pr.shape[0]
            out = torch.empty((n, self.spec.embed_dim), dtype=torch.float16, device=self.device)
            a.n, a.seq_len, a.normalize, a.out_f16 = n, sl, int(g.get("normalize", 0)), _ptr(out).value
            outs.append(out)
        self._ck(self.lib.ovmr_encode_text_groups(self.h, arr, len(groups), _stream()), "ovmr_encode_text_groups")
        return outs

    def encode_text_ensemble(self, ids: torch.Tensor, seq_lens=None) -> torch.Tensor:
        """The prompt-ensembled text classifier of ZeroshotCLIP2 (ovmr_encode_text_ensemble): ids [T, C, context_length], template-major
        -> [C, embed_dim] fp16.  seq_lens: T template lengths; None = each template's exact length (max EOT position + 1) when `ids` is a
        host tensor, the full context otherwise (no device read-back here)."""
        self._want_ids("encode_text_ensemble", "ids", ids, (None, None, self.spec.context_length))
        if isinstance(ids, np.ndarray):
            ids = torch.from_numpy(ids)
        T, C = int(ids.shape[0]), int(ids.shape[1])
        if seq_lens is not None and len(seq_lens) != T:
            _refuse("encode_text_ensemble", "seq_lens", f"{T} lengths, one for each of the templates in ids {list(ids.shape)}", f"{len(seq_lens)}")
        if not ids.is_cuda and ids.numel():
            eot = ids.argmax(dim=-1).amax(dim=1)          # EOT has the largest id (clip/model.py:831)
            if seq_lens is None:
                seq_lens = (eot + 1).tolist()
            elif any(int(e) >= int(s) for e, s in zip(eot.tolist(), seq_lens)):
                raise ValueError(f"seq_lens {list(seq_lens)} do not reach the EOT tokens at {eot.tolist()}")
        sl = None
        if seq_lens is not None:
            sl = (ctypes.c_int32 * max(1, T))(*[int(s) for s in seq_lens])
        ids = self._dev(ids, torch.int64)
        out = torch.empty((C, self.spec.embed_dim), dtype=torch.float16, device=self.device)
        self._ck(self.lib.ovmr_encode_text_ensemble(self.h, _ptr(ids), T, C, sl, _ptr(out), _stream()), "ovmr_encode_text_ensemble")
        return out

    def embed_tokens(self, ids: torch.Tensor) -> torch.Tensor:
        """ids [N, L] (host ids are held to [0, vocab_size)) -> [N, L, transformer_width] fp16."""
        self._want_ids("embed_tokens", "ids", ids, (None, None))
        ids = self._dev(ids, torch.int64)
        N, L = ids.shape
        out = torch.empty((N, L, self.spec.transformer_width), dtype=torch.float16, device=self.device)
        self._ck(self.lib.ovmr_embed_tokens(self.h, _ptr(ids), N, L, _ptr(out), _stream()), "ovmr_embed_tokens")
        return out

    def generate_tokens(self, feats: torch.Tensor) -> torch.Tensor:
        """feats [Cb, S, embed_dim] -> tokens [Cb, n_ctx, embed_dim] fp32."""
        _want("generate_tokens", "feats", feats, (None, None, self.spec.embed_dim))
        feats = self._dev(feats, torch.float16)
        Cb, S, D = feats.shape
        out = torch.empty((Cb, self.n_ctx, D), dtype=torch.float32, device=self.device)
        self._ck(self.lib.ovmr_generate_tokens(self.h, _ptr(feats), Cb, S, _ptr(out), _stream()), "ovmr_generate_tokens")
        return out

    def generate_tokens_ragged(self, feats: torch.Tensor, shots) -> torch.Tensor:
        """ovmr_generate_tokens_ragged: feats [R, embed_dim], class after class, class c owning shots[c] rows -> tokens [Cb, n_ctx, D] fp32, each
        class bit-identical to generate_tokens on its rows alone.  `shots` is a HOST sequence (list, numpy array or CPU tensor): the
        library's host array and the kernels' device prefix sum are both built here from this ONE list, so they cannot disagree."""
        if isinstance(shots, torch.Tensor):
            if shots.is_cuda:
                raise ValueError("shots must live on the host: the library plans its launches from them")
            shots = shots.tolist()
        shots = [int(n) for n in shots]
        _want("generate_tokens_ragged", "feats", feats, (None, self.spec.embed_dim))
        feats = self._dev(feats, torch.float16)
        Cb, (R, D) = len(shots), feats.shape
        host = (ctypes.c_int32 * max(1, Cb))(*shots)
        offsets = self._dev(np.concatenate([[0], np.cumsum(np.asarray(shots, dtype=np.int64))]).astype(np.int32))
        out = torch.empty((Cb, self.n_ctx, D), dtype=torch.float32, device=self.device)
        self._ck(self.lib.ovmr_generate_tokens_ragged(self.h, _ptr(feats), host, _ptr(offsets), Cb, R, _ptr(out), _stream()),
                 "ovmr_generate_tokens_ragged")
        return out

    def assemble_prompts(self, base: torch.Tensor, labels: Optional[torch.Tensor], tokens: torch.Tensor) -> torch.Tensor:
        """base [rows, context_length, transformer_width], tokens [Cb, n_ctx, transformer_width], labels [Cb] (the row of base each class
        takes; host labels are held to base's rows) or None (row 0 for every class) -> [Cb, context_length, transformer_width] fp16."""
        sp = self.spec
        _want("assemble_prompts", "tokens", tokens, (None, self.n_ctx, sp.transformer_width))
        _want("assemble_prompts", "base", base, (None, sp.context_length, sp.transformer_width), at_least=1)
        if labels is not None:
            _want("assemble_prompts", "labels", labels, (tokens.shape[0],))
            _want_range("assemble_prompts", "labels", labels, 0, int(base.shape[0]), "rows of base")
        base = self._dev(base, torch.float16)
        tokens = self._dev(tokens, torch.float32)
        labels = None if labels is None else self._dev(labels, torch.int64)
        Cb = tokens.shape[0]
        out = torch.empty((Cb, self.spec.context_length, self.spec.transformer_width), dtype=torch.float16, device=self.device)
        self._ck(self.lib.ovmr_assemble_prompts(self.h, _ptr(base), _ptr(labels), _ptr(tokens), Cb, _ptr(out), _stream()),
                 "ovmr_assemble_prompts")
        return out

    def xval_counts(self, feats: torch.Tensor, labels: torch.Tensor, clf: torch.Tensor,
                    tp: torch.Tensor, n_pred: torch.Tensor):
        """feats [R, embed_dim], labels [R], clf [C, embed_dim]; tp and n_pred accumulate in place: int32, contiguous, on the engine's
        device, at least C elements each."""
        D = self.spec.embed_dim
        _want("xval_counts", "feats", feats, (None, D))
        _want("xval_counts", "labels", labels, (feats.shape[0],))
        _want("xval_counts", "clf", clf, (None, D))
        for name, x in (("tp", tp), ("n_pred", n_pred)):
            _want("xval_counts", name, x, None, torch.int32, self.device, dense=True, at_least=int(clf.shape[0]))
        feats = self._dev(feats, torch.float16)
        labels = self._dev(labels, torch.int32)
        clf = self._dev(clf, torch.float16)
        self._ck(self.lib.ovmr_xval_counts(self.h, _ptr(feats), _ptr(labels), feats.shape[0], _ptr(clf), clf.shape[0],
                                           _ptr(tp), _ptr(n_pred), _stream()), "ovmr_xval_counts")

    def fusion_weights(self, counts: torch.Tensor, n_label: torch.Tensor, tau: float) -> torch.Tensor:
        """counts [3, 2, C], n_label [C] -> [C, 3] fp32."""
        _want("fusion_weights", "n_label", n_label, (None,))
        _want("fusion_weights", "counts", counts, (3, 2, n_label.shape[0]))
        counts = self._dev(counts, torch.int32)
        n_label = self._dev(n_label, torch.int32)
        C = n_label.shape[0]
        out = torch.empty((C, 3), dtype=torch.float32, device=self.device)
        self._ck(self.lib.ovmr_fusion_weights(self.h, _ptr(counts), _ptr(n_label), C, float(tau), _ptr(out), _stream()),
                 "ovmr_fusion_weights")
        return out

    def pack_rows(self, mm, v, t, tokens, labels, bound: int) -> torch.Tensor:
        """One rank's block of the sharded job's all-gather (ovmr_amd/shard.py pack_block, one launch): rows `labels` of the class-indexed
        fp16 buffers mm / v / t [C, D] and tokens [C, n_ctx, D] + the label bits, [bound, 3 D + n_ctx D + 2] fp16.  The four buffers go to
        the library as they are: fp16, contiguous, on the engine's device; labels [n], n <= bound."""
        _want("pack_rows", "mm", mm, (None, None))
        _want("pack_rows", "tokens", tokens, (mm.shape[0], None, mm.shape[1]))
        _want("pack_rows", "labels", labels, (None,))
        n, (C, D), n_ctx = int(labels.shape[0]), mm.shape, tokens.shape[1]
        if n > bound:
            raise RuntimeError(f"this rank produced {n} classes, more than the bound {bound} every rank agreed on: the eval-set "
                               "loader yields more than TEST.BATCH_SIZE // NUM_SHOTS classes per batch")
        if D % 2:
            _refuse("pack_rows", "mm", "of even width (the label takes two fp16 columns)", f"{list(mm.shape)}")
        for name, x, shape in (("mm", mm, (C, D)), ("v", v, (C, D)), ("t", t, (C, D)), ("tokens", tokens, (C, n_ctx, D))):
            _want("pack_rows", name, x, shape, torch.float16, self.device, dense=True)
        labels = self._dev(labels, torch.int64)
        block = torch.empty((bound, (3 + n_ctx) * D + 2), dtype=torch.float16, device=self.device)
        self._ck(self.lib.ovmr_pack_rows(_ptr(mm), _ptr(v), _ptr(t), _ptr(tokens), _ptr(labels), n, D, n_ctx, bound, _ptr(block), _stream()),
                 "ovmr_pack_rows")
        return block

    def unpack_rows(self, gathered: torch.Tensor, C: int, D: int, n_ctx: int):
        """The gathered blocks of all ranks, [rows, (3 + n_ctx) D + 2] -> (mm, v, t [C, D], tokens [C, n_ctx, D], seen int32 [C + 1]); one launch (each result owns its storage: they are saved to files)."""
        _want("unpack_rows", "gathered", gathered, (None, (3 + n_ctx) * D + 2))
        gathered = self._dev(gathered, torch.float16)
        z = dict(dtype=torch.float16, device=self.device)                                      # (a class no rank sent stays zero; seen says so)
        mm, v, t, tokens = torch.zeros((C, D), **z), torch.zeros((C, D), **z), torch.zeros((C, D), **z), torch.zeros((C, n_ctx, D), **z)
        seen = torch.zeros(C + 1, dtype=torch.int32, device=self.device)
        self._ck(self.lib.ovmr_unpack_rows(_ptr(gathered), gathered.shape[0], C, D, n_ctx, _ptr(mm), _ptr(v), _ptr(t), _ptr(tokens), _ptr(seen),
                                           _stream()), "ovmr_unpack_rows")
        return mm, v, t, tokens, seen

    def _want_head(self, where: str, feats, clf, w) -> tuple:
        """feats [B, embed_dim]; the classifiers that are given [C, embed_dim], one C for all; w [C, 3] when given.  Returns (B, C)."""
        D = self.spec.embed_dim
        _want(where, "feats", feats, (None, D))
        given = [(n, x) for n, x in clf if x is not None]
        if not given:
            _refuse(where, "mm / v / t", "at least one classifier", "None for all three")
        _want(where, given[0][0], given[0][1], (None, D))
        C = int(given[0][1].shape[0])
        for n, x in given[1:]:
            _want(where, n, x, (C, D))
        if w is not None:
            _want(where, "w", w, (C, 3))
        return int(feats.shape[0]), C

    def fused_logits(self, feats, mm, v, t, w, mode: str = "fusion", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """feats [B, embed_dim]; mm / v / t [C, embed_dim] (None where the mode does not read one); w [C, 3] or None -> [B, C] fp32; out,
        when given: that tensor, fp32, contiguous, on the engine's device."""
        B, C = self._want_head("fused_logits", feats, (("mm", mm), ("v", v), ("t", t)), w)
        if out is not None:
            _want("fused_logits", "out", out, (B, C), torch.float32, self.device, dense=True)
        feats = self._dev(feats, torch.float16)
        cl = [None if x is None else self._dev(x, torch.float16) for x in (mm, v, t)]
        w = None if w is None else self._dev(w, torch.float32)
        if out is None:
            out = torch.empty((B, C), dtype=torch.float32, device=self.device)
        self._ck(self.lib.ovmr_fused_logits(self.h, _ptr(feats), B, _ptr(cl[0]), _ptr(cl[1]), _ptr(cl[2]),
                                            _ptr(w), C, MODES[mode], _ptr(out), _stream()), "ovmr_fused_logits")
        return out

    def fused_logits_all(self, feats, mm, v, t, w, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The four eval modes of one batch from one pass over the head (ovmr_fused_logits_all): [4, B, C] fp32 in ALL_MODES order, plane p
        bit-equal to fused_logits(mode = ALL_MODES[p]).  feats [B, embed_dim], mm / v / t [C, embed_dim], w [C, 3], all required.  `out`
        may be a row slice big[:, r0:r1] of a contiguous [4, Btot, C] tensor: fp32 on the engine's device, dense [B, C] planes."""
        for name, x in (("mm", mm), ("v", v), ("t", t), ("w", w)):
            if x is None:
                _refuse("fused_logits_all", name, "given (all three classifiers and w are read)", "None")
        B, C = self._want_head("fused_logits_all", feats, (("mm", mm), ("v", v), ("t", t)), w)
        if out is not None:
            _want("fused_logits_all", "out", out, (4, B, C), torch.float32, self.device)
            if B and not (out.stride(2) == 1 and out.stride(1) == C and out.stride(0) >= B * C):
                _refuse("fused_logits_all", "out", f"dense [{B}, {C}] planes, at least {B * C} elements apart",
                        f"strides {tuple(out.stride())}")
        feats = self._dev(feats, torch.float16)
        mm, v, t = (self._dev(x, torch.float16) for x in (mm, v, t))
        w = self._dev(w, torch.float32)
        if out is None:
            out = torch.empty((4, B, C), dtype=torch.float32, device=self.device)
        self._ck(self.lib.ovmr_fused_logits_all(self.h, _ptr(feats), B, _ptr(mm), _ptr(v), _ptr(t), _ptr(w), C, _ptr(out),
                                                out.stride(0) if B else 0, _stream()), "ovmr_fused_logits_all")
        return out

    def head_plan(self, B: int, C: int) -> int:
        """1: fused_logits runs the one-launch head for B rows x C classes, 0: the GEMM path (their logits may differ by one fp16 step)."""
        return int(self.lib.ovmr_head_plan(self.h, int(B), int(C)))

    def zeroshot_logits(self, feats, text_feats, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """feats [B, embed_dim], text_feats [C, embed_dim] -> [B, C] fp16; out, when given: that tensor, fp16, contiguous, on the engine's
        device."""
        D = self.spec.embed_dim
        _want("zeroshot_logits", "feats", feats, (None, D))
        _want("zeroshot_logits", "text_feats", text_feats, (None, D))
        B, C = int(feats.shape[0]), int(text_feats.shape[0])
        if out is not None:
            _want("zeroshot_logits", "out", out, (B, C), torch.float16, self.device, dense=True)
        feats = self._dev(feats, torch.float16)
        text_feats = self._dev(text_feats, torch.float16)
        if out is None:
            out = torch.empty((B, C), dtype=torch.float16, device=self.device)
        self._ck(self.lib.ovmr_zeroshot_logits(self.h, _ptr(feats), B, _ptr(text_feats), C, _ptr(out), _stream()), "ovmr_zeroshot_logits")
        return out
