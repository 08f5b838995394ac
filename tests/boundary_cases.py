"""The Python boundary of libovmr_hip.so, stated once: what every pointer argument of the C ABI must cover, and the calls the wrappers of
ovmr_amd (runtime.Engine, runtime.topk_rows / eval_detail, evaluator.Classification.process, loader.preprocess_u8) must take or refuse.

The library sees an address and a few integers, never a tensor (include/ovmr_hip.h).  ABI restates FROM THE HEADER, per entry point, how many
elements of which dtype each pointer must cover, as a function of the scalar arguments of the same call and of the handle's geometry
(ModelSpec + n_ctx).  ACCEPTED lists well-formed calls in the plain layout and in every layout the wrappers repair or take as they are;
VIOLATIONS lists calls with ONE operand wrong, with the name of the argument the refusal has to name.  tests/test_boundary_cpu.py runs both
tables against a recording stand-in for the library (no GPU, no library); tests/test_hip_boundary.py runs the accepted layouts on the GPU
against the same call on plain contiguous operands, bit for bit.  Plain Python: importing this file needs neither."""
import ctypes
import zlib
from collections import namedtuple

import numpy as np
import torch

from ovmr_amd import synth

Geo = namedtuple("Geo", "R ctx width embed n_ctx vocab")
SPEC = synth.SPECS["tiny"]
N_CTX = 2
TINY = Geo(SPEC.image_resolution, SPEC.context_length, SPEC.transformer_width, SPEC.embed_dim, N_CTX, SPEC.vocab_size)
assert TINY == Geo(32, 77, 128, 128, 2, 49408)

F16, F32, I64, I32, U8 = "f16", "f32", "i64", "i32", "u8"
TORCH = {F16: torch.float16, F32: torch.float32, I64: torch.int64, I32: torch.int32, U8: torch.uint8}
FLOAT_OF = {0: F16, 1: F32}                       # enum { OVMR_F16 = 0, OVMR_F32 = 1, ... }: the `dtype` argument of an entry point


def _p(x):
    """A pointer argument as an address (None = NULL)."""
    return x.value if isinstance(x, ctypes.c_void_p) else x


# --------------------------------------------------------------------------------------------------------------- the header, restated
# entry point -> f(geometry, the call's arguments as the library receives them, handle and stream included) -> one line per pointer:
# (argument, address, dtype, elements it must cover).  A NULL the header allows gives no line; "rows" marks outputs [B, C] with a row stride.

def _text_group_lines(g, grp):
    if grp.ids:
        lines = [("ids", grp.ids, I64, grp.n * g.ctx)]
    else:
        lines = [("prompts", grp.prompts_f16, F16, grp.n * g.ctx * g.width), ("index", grp.index, I32, grp.n)]
    return lines + [("out", grp.out_f16, F16, grp.n * g.embed)]


def _rows(a_out, dt, ld, B, C):
    return ("outputs", _p(a_out), FLOAT_OF[dt], ((B - 1) * ld + C) if B else 0)


NULLABLE = {"ovmr_assemble_prompts": {"labels"}, "ovmr_fused_logits": {"mm", "v", "t", "w"}, "ovmr_topk_rows": {"values", "labels", "hits"},
            "ovmr_eval_detail": {"hits", "class_hits", "cmat"}}

ABI = {
    "ovmr_set_weight": lambda g, a: [("data", _p(a[2]), FLOAT_OF[a[3]], int(np.prod([a[5][i] for i in range(a[4])], dtype=np.int64)))],
    "ovmr_encode_image": lambda g, a: [("image", _p(a[1]), FLOAT_OF[a[2]], a[3] * 3 * g.R * g.R), ("out", _p(a[4]), F16, a[3] * g.embed)],
    "ovmr_encode_text_embedded": lambda g, a: [("prompts", _p(a[1]), F16, a[3] * g.ctx * g.width), ("index", _p(a[2]), I32, a[3]),
                                               ("out", _p(a[5]), F16, a[3] * g.embed)],
    "ovmr_encode_text_ids": lambda g, a: [("ids", _p(a[1]), I64, a[2] * g.ctx), ("out", _p(a[4]), F16, a[2] * g.embed)],
    "ovmr_encode_text_groups": lambda g, a: [l for k in range(a[2]) for l in _text_group_lines(g, a[1][k])],
    "ovmr_encode_text_ensemble": lambda g, a: [("ids", _p(a[1]), I64, a[2] * a[3] * g.ctx), ("out", _p(a[5]), F16, a[3] * g.embed)],
    "ovmr_embed_tokens": lambda g, a: [("ids", _p(a[1]), I64, a[2] * a[3]), ("out", _p(a[4]), F16, a[2] * a[3] * g.width)],
    "ovmr_generate_tokens": lambda g, a: [("feats", _p(a[1]), F16, a[2] * a[3] * g.embed), ("tokens", _p(a[4]), F32, a[2] * g.n_ctx * g.embed)],
    "ovmr_generate_tokens_ragged": lambda g, a: [("feats", _p(a[1]), F16, a[5] * g.embed), ("offsets", _p(a[3]), I32, a[4] + 1),
                                                 ("tokens", _p(a[6]), F32, a[4] * g.n_ctx * g.embed)],
    # base: [*, context_length, width] -- the header does not say how many rows; row 0 is read when labels is NULL
    "ovmr_assemble_prompts": lambda g, a: [("base", _p(a[1]), F16, g.ctx * g.width if a[4] else 0), ("labels", _p(a[2]), I64, a[4]),
                                           ("tokens", _p(a[3]), F32, a[4] * g.n_ctx * g.width), ("out", _p(a[5]), F16, a[4] * g.ctx * g.width)],
    "ovmr_xval_counts": lambda g, a: [("feats", _p(a[1]), F16, a[3] * g.embed), ("labels", _p(a[2]), I32, a[3]), ("clf", _p(a[4]), F16, a[5] * g.embed),
                                      ("tp", _p(a[6]), I32, a[5]), ("n_pred", _p(a[7]), I32, a[5])],
    "ovmr_fusion_weights": lambda g, a: [("counts", _p(a[1]), I32, 3 * 2 * a[3]), ("n_label", _p(a[2]), I32, a[3]), ("out", _p(a[5]), F32, a[3] * 3)],
    "ovmr_fused_logits": lambda g, a: [("feats", _p(a[1]), F16, a[2] * g.embed), ("mm", _p(a[3]), F16, a[7] * g.embed), ("v", _p(a[4]), F16, a[7] * g.embed),
                                       ("t", _p(a[5]), F16, a[7] * g.embed), ("w", _p(a[6]), F32, a[7] * 3), ("out", _p(a[9]), F32, a[2] * a[7])],
    # four planes [B, C] at plane_stride: the last one ends at 3 * plane_stride + B * C
    "ovmr_fused_logits_all": lambda g, a: [("feats", _p(a[1]), F16, a[2] * g.embed), ("mm", _p(a[3]), F16, a[7] * g.embed), ("v", _p(a[4]), F16, a[7] * g.embed),
                                           ("t", _p(a[5]), F16, a[7] * g.embed), ("w", _p(a[6]), F32, a[7] * 3),
                                           ("out planes", _p(a[8]), F32, (3 * a[9] + a[2] * a[7]) if a[2] else 0)],
    "ovmr_zeroshot_logits": lambda g, a: [("feats", _p(a[1]), F16, a[2] * g.embed), ("text", _p(a[3]), F16, a[4] * g.embed), ("out", _p(a[5]), F16, a[2] * a[4])],
    # (no handle) mm / v / t [C, D] and tokens [C, n_ctx, D] are class-indexed: C is not an argument, a gathered row needs one row at least
    "ovmr_pack_rows": lambda g, a: [("mm", _p(a[0]), F16, a[6] if a[5] else 0), ("v", _p(a[1]), F16, a[6] if a[5] else 0), ("t", _p(a[2]), F16, a[6] if a[5] else 0),
                                    ("tokens", _p(a[3]), F16, a[7] * a[6] if a[5] else 0), ("labels", _p(a[4]), I64, a[5]),
                                    ("block", _p(a[9]), F16, a[8] * ((3 + a[7]) * a[6] + 2))],
    "ovmr_unpack_rows": lambda g, a: [("gathered", _p(a[0]), F16, a[1] * ((3 + a[4]) * a[3] + 2)), ("mm", _p(a[5]), F16, a[2] * a[3]), ("v", _p(a[6]), F16, a[2] * a[3]),
                                      ("t", _p(a[7]), F16, a[2] * a[3]), ("tokens", _p(a[8]), F16, a[2] * a[4] * a[3]), ("seen", _p(a[9]), I32, a[2] + 1)],
    "ovmr_eval_counts": lambda g, a: [_rows(a[0], a[1], a[2], a[4], a[5]), ("labels", _p(a[3]), I64, a[4]), ("counts", _p(a[6]), I32, 3 * a[5] + 1)],
    "ovmr_topk_rows": lambda g, a: [_rows(a[0], a[1], a[2], a[3], a[4]), ("values", _p(a[6]), F32, a[3] * a[5]), ("indices", _p(a[7]), I32, a[3] * a[5]),
                                    ("labels", _p(a[8]), I64, a[3]), ("hits", _p(a[9]), I32, 1)],
    "ovmr_eval_detail": lambda g, a: [_rows(a[0], a[1], a[2], a[4], a[5]), ("labels", _p(a[3]), I64, a[4]), ("counts", _p(a[7]), I32, 3 * a[5] + 1),
                                      ("hits", _p(a[8]), I32, 1), ("class_hits", _p(a[9]), I32, a[5]), ("cmat", _p(a[10]), I32, a[5] * a[5])],
    "ovmr_preprocess_u8": lambda g, a: [("u8", _p(a[0]), U8, a[1] * a[2] * a[2] * 3), ("out", _p(a[5]), F16, a[1] * 3 * a[2] * a[2])],
}
STRIDED = {"outputs", "out planes"}              # the header gives these a row / plane stride: every other operand is dense

# What the header says about the scalars themselves, beyond the counts above.
SCALARS = {
    "ovmr_fused_logits_all": lambda g, a: a[9] >= a[2] * a[7],                  # plane_stride >= B * C
    "ovmr_eval_counts": lambda g, a: a[4] == 0 or a[2] >= a[5],                 # ld >= C
    "ovmr_topk_rows": lambda g, a: a[3] == 0 or a[2] >= a[4],
    "ovmr_eval_detail": lambda g, a: a[4] == 0 or a[2] >= a[5],
    "ovmr_preprocess_u8": lambda g, a: a[2] % 8 == 0,                           # R % 8 == 0
    "ovmr_pack_rows": lambda g, a: a[6] % 2 == 0 and a[5] <= a[8],              # D even, n <= bound
    "ovmr_encode_text_ids": lambda g, a: 1 <= a[3] <= g.ctx,                    # seq_len <= context_length
    "ovmr_encode_text_embedded": lambda g, a: 1 <= a[4] <= g.ctx,
}

# Entry points that take no device address from a caller's tensor, by name: a new entry point fails tests/test_boundary_cpu.py until it is
# put here or into ABI.
EXEMPT = {
    # handle-only and pure-integer entry points
    "ovmr_create", "ovmr_destroy", "ovmr_last_error", "ovmr_version", "ovmr_set_option", "ovmr_finalize", "ovmr_head_plan", "ovmr_logit_scale",
    "ovmr_encode_chunk", "ovmr_encode_plan", "ovmr_flops_per_image", "ovmr_flops_per_image_executed", "ovmr_flops_executed",
    "ovmr_flops_per_prompt", "ovmr_debug_attention_route", "ovmr_debug_gemm_route", "ovmr_debug_gemm_tile_kernels",
    "ovmr_debug_fill_workspace",
    # loader.DeviceResizer.run hands in buffers it sizes from its own plan (ovmr_amd/resize.py): no caller's tensor shape is involved
    "ovmr_resize_crop_u8",
    # the kernel-test hooks have no wrapper in the package: the tests that call them size their operands themselves
    "ovmr_debug_gemm", "ovmr_debug_lnfold", "ovmr_debug_layernorm", "ovmr_debug_attention", "ovmr_debug_l2norm", "ovmr_debug_text_ensemble",
    "ovmr_debug_text_embed_ids", "ovmr_debug_text_add_pos", "ovmr_debug_gather_rows", "ovmr_debug_im2col", "ovmr_debug_fill_cls",
    "ovmr_debug_gemm_patches", "ovmr_debug_gemm_strided", "ovmr_debug_attention_f32_varlen", "ovmr_debug_attention_f32_long",
    "ovmr_debug_attention_q",
}


def extent(t: torch.Tensor) -> int:
    """Elements from t's first element to its last one, in storage order: what an address taken from t covers."""
    return 0 if t.numel() == 0 else 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))


class Recorder:
    """Stands where the library stands: records every call, returns success.  With `forward` (the real library) the call goes on to it."""

    def __init__(self, forward=None):
        self.calls, self.forward = [], forward

    def __getattr__(self, name):
        if not name.startswith("ovmr_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            if self.forward is not None:
                return getattr(self.forward, name)(*args)
            return {"ovmr_last_error": b"", "ovmr_logit_scale": 100.0}.get(name, 0)
        return call

    def launches(self):
        return [(n, a) for n, a in self.calls if n in ABI]


def check_call(entry, args, held, geo=TINY):
    """One recorded call against the header: every address belongs to a tensor the wrapper handed over (held: address -> tensor, kept by
    the patched runtime._ptr), of the dtype the header names, dense unless the header gives it a stride, covering the element count the
    header derives from THIS call's scalars.  Returns the problems found."""
    bad = []
    if entry in SCALARS and not SCALARS[entry](geo, args):
        bad.append(f"{entry}: the scalar arguments {[x for x in args if isinstance(x, int)]} break the header's condition")
    for name, addr, dtype, count in ABI[entry](geo, args):
        if addr is None or addr == 0:
            if count > 0 and name not in NULLABLE.get(entry, ()):
                bad.append(f"{entry}: {name} is NULL, the call needs {count} elements")
            continue
        t = held.get(addr)
        if t is None:
            bad.append(f"{entry}: the address of {name} did not come through runtime._ptr")
            continue
        if t.dtype != TORCH[dtype]:
            bad.append(f"{entry}: {name} is {t.dtype}, the header names {dtype}")
        if name not in STRIDED and not t.is_contiguous():
            bad.append(f"{entry}: {name} is not contiguous (strides {t.stride()})")
        if extent(t) < count:
            bad.append(f"{entry}: {name} covers {extent(t)} elements, the call's scalars need {count}")
    return bad


# ------------------------------------------------------------------------------------------------------------------------------ data
def _rng(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


def _f(tag, *shape, dtype=torch.float32, scale=1.0):
    return torch.from_numpy((_rng(tag).standard_normal(shape) * scale).astype(np.float32)).to(dtype)


def _unit(tag, n, d=TINY.embed):
    x = _f(tag, n, d)
    return (x / x.norm(dim=-1, keepdim=True).clamp_min(1e-6)).half()


def _ids(n, seed=4321):
    return torch.from_numpy(synth.class_token_ids(n, seed=seed))


def _ints(tag, n, hi, dtype=torch.int64):
    return torch.from_numpy(_rng(tag).integers(0, max(1, hi), n)).to(dtype)


# layouts: x is the plain host tensor, the result is what the caller hands in
def offset(x, dev):
    """big[1:1 + n]: a non-zero storage offset."""
    big = torch.cat([x[:1], x, x[:1]]).to(dev) if len(x) else torch.cat([x.new_zeros((1,) + x.shape[1:]), x]).to(dev)
    return big[1:1 + len(x)]


def transposed(x, dev, d0=-2, d1=-1):
    return x.transpose(d0, d1).contiguous().to(dev).transpose(d0, d1)


def expanded(x, dev):
    return x[:1].to(dev).expand(x.shape[0], *([-1] * (x.dim() - 1)))


LAYOUTS = {"offset": offset, "transposed": transposed, "expanded": expanded, "numpy": lambda x, dev: x.numpy(), "host": lambda x, dev: x,
           "channels_last": lambda x, dev: x.to(dev).contiguous(memory_format=torch.channels_last),
           "hw_transposed": lambda x, dev: transposed(x, dev, -2, -1)}
for _n, _dt in (("fp64", torch.float64), ("fp16", torch.float16), ("fp32", torch.float32), ("int32", torch.int32), ("int64", torch.int64)):
    LAYOUTS[_n] = (lambda dt: lambda x, dev: x.to(dev).to(dt))(_dt)


def _as(dtype):
    return lambda x, dev: torch.as_tensor(x).to(dev).to(TORCH[dtype]).clone(memory_format=torch.contiguous_format)


def _image_plain(x, dev):
    x = torch.as_tensor(x)
    return x.to(dev).to(x.dtype if x.dtype in (torch.float16, torch.float32) else torch.float32).clone(memory_format=torch.contiguous_format)


def _groups_plain(groups, dev):
    return [{k: (PLAIN["encode_text_embedded" if k != "ids" else "encode_text_ids"][k](v, dev) if k in ("ids", "prompts", "index") else v)
             for k, v in g.items()} for g in groups]


def _rows_plain(x, dev):
    x = x.to(dev)
    return x.to(x.dtype if x.dtype in (torch.float16, torch.float32) else torch.float32).clone(memory_format=torch.contiguous_format)


# wrapper -> operand -> how the same call is made "on .contiguous() operands of the target dtype" (operands not named go as they are)
_HEAD = {"feats": _as(F16), "mm": _as(F16), "v": _as(F16), "t": _as(F16), "w": _as(F32)}
PLAIN = {
    "set_weight": {"tensor": _image_plain},
    "encode_image": {"image": _image_plain},
    "encode_text_embedded": {"prompts": _as(F16), "index": _as(I32)},
    "encode_text_ids": {"ids": _as(I64)},
    "encode_text_groups": {"groups": _groups_plain},
    "encode_text_ensemble": {"ids": _as(I64)},
    "embed_tokens": {"ids": _as(I64)},
    "generate_tokens": {"feats": _as(F16)},
    "generate_tokens_ragged": {"feats": _as(F16)},
    "assemble_prompts": {"base": _as(F16), "labels": _as(I64), "tokens": _as(F32)},
    "xval_counts": {"feats": _as(F16), "labels": _as(I32), "clf": _as(F16), "tp": _as(I32), "n_pred": _as(I32)},
    "fusion_weights": {"counts": _as(I32), "n_label": _as(I32)},
    "fused_logits": _HEAD, "fused_logits_all": _HEAD,
    "zeroshot_logits": {"feats": _as(F16), "text_feats": _as(F16)},
    "pack_rows": {"mm": _as(F16), "v": _as(F16), "t": _as(F16), "tokens": _as(F16), "labels": _as(I64)},
    "unpack_rows": {"gathered": _as(F16)},
    "eval_counts": {"mo": _rows_plain, "gt": _as(I64)},
    "topk_rows": {"mo": _rows_plain, "labels": _as(I64), "hits": _as(I32)},
    "eval_detail": {"mo": _rows_plain, "labels": _as(I64), "counts": _as(I32), "hits": _as(I32), "class_hits": _as(I32), "cmat": _as(I32)},
    "preprocess_u8": {"u8": _as(U8)},
}
ENTRY = {w: "ovmr_" + w for w in PLAIN}
DEVICE_ONLY = {"eval_counts", "topk_rows", "eval_detail", "preprocess_u8"}    # these refuse host tensors: no stand-in device on a CPU box


def plain_of(wrapper, ops, dev):
    """The same call on contiguous operands of the target dtype on `dev`, every tensor a fresh copy, no caller's `out`."""
    return {k: (PLAIN[wrapper][k](x, dev) if k in PLAIN[wrapper] and x is not None else x) for k, x in ops.items() if k != "out"}


def _kw(o, *names):
    return {k: o[k] for k in names if k in o}


def _process(_, o):
    from ovmr_amd.evaluator import Classification
    ev = Classification(C, device=o["mo"].device)
    ev.process(o["mo"], o["gt"])
    return ev._counts


def _preprocess(_, o):
    from ovmr_amd import loader
    return loader.preprocess_u8(o["u8"], **_kw(o, "out", "mean", "std"))


def _topk(_, o):
    from ovmr_amd import runtime
    v, i = runtime.topk_rows(o["mo"], o["k"], o.get("labels"), o.get("hits"))
    return (v, i) + ((o["hits"],) if o.get("hits") is not None else ())


def _detail(_, o):
    from ovmr_amd import runtime
    runtime.eval_detail(o["mo"], o["labels"], o["k"], o["counts"], o.get("hits"), o.get("class_hits"), o.get("cmat"))
    return tuple(o[k] for k in ("counts", "hits", "class_hits", "cmat") if o.get(k) is not None)


def _xval(e, o):
    e.xval_counts(o["feats"], o["labels"], o["clf"], o["tp"], o["n_pred"])
    return o["tp"], o["n_pred"]


# wrapper -> f(engine, operands) -> the tensors the call produced (accumulators included)
CALLS = {
    "set_weight": lambda e, o: e.set_weight(o["name"], o["tensor"]),
    "encode_image": lambda e, o: e.encode_image(o["image"], **_kw(o, "normalize", "out")),
    "encode_text_embedded": lambda e, o: e.encode_text_embedded(o["prompts"], o["index"], **_kw(o, "seq_len", "normalize")),
    "encode_text_ids": lambda e, o: e.encode_text_ids(o["ids"], **_kw(o, "seq_len", "normalize")),
    "encode_text_groups": lambda e, o: tuple(e.encode_text_groups(o["groups"])),
    "encode_text_ensemble": lambda e, o: e.encode_text_ensemble(o["ids"], **_kw(o, "seq_lens")),
    "embed_tokens": lambda e, o: e.embed_tokens(o["ids"]),
    "generate_tokens": lambda e, o: e.generate_tokens(o["feats"]),
    "generate_tokens_ragged": lambda e, o: e.generate_tokens_ragged(o["feats"], o["shots"]),
    "assemble_prompts": lambda e, o: e.assemble_prompts(o["base"], o["labels"], o["tokens"]),
    "xval_counts": _xval,
    "fusion_weights": lambda e, o: e.fusion_weights(o["counts"], o["n_label"], o["tau"]),
    "fused_logits": lambda e, o: e.fused_logits(o["feats"], o["mm"], o["v"], o["t"], o["w"], **_kw(o, "mode", "out")),
    "fused_logits_all": lambda e, o: e.fused_logits_all(o["feats"], o["mm"], o["v"], o["t"], o["w"], **_kw(o, "out")),
    "zeroshot_logits": lambda e, o: e.zeroshot_logits(o["feats"], o["text_feats"], **_kw(o, "out")),
    "pack_rows": lambda e, o: e.pack_rows(o["mm"], o["v"], o["t"], o["tokens"], o["labels"], o["bound"]),
    "unpack_rows": lambda e, o: e.unpack_rows(o["gathered"], o["C"], o["D"], o["n_ctx"]),
    "eval_counts": _process, "topk_rows": _topk, "eval_detail": _detail, "preprocess_u8": _preprocess,
}

# ------------------------------------------------------------------------------------------------------ the well-formed operands
E, W, CTX, R = TINY.embed, TINY.width, TINY.ctx, TINY.R
B, N, C, CB, S = 3, 3, 5, 3, 4                       # images, prompts, classes, classes of a generator call, shots


def _head(dev, b=B, c=C):
    return {"feats": _unit("hf", b).to(dev), "mm": _unit("hmm", c).to(dev), "v": _unit("hv", c).to(dev), "t": _unit("ht", c).to(dev),
            "w": torch.softmax(_f("hw", c, 3), -1).to(dev)}


def _packed(dev, n=3, c=C, bound=4):
    return {"mm": _unit("pm", c).to(dev), "v": _unit("pv", c).to(dev), "t": _unit("pt", c).to(dev), "tokens": _f("ptk", c, N_CTX, E, dtype=torch.float16).to(dev),
            "labels": torch.tensor([4, 0, 2, 1, 3][:n], dtype=torch.int64).to(dev), "bound": bound}


def _gathered(dev, rows=6, c=C):
    g = _f("gath", rows, (3 + N_CTX) * E + 2, dtype=torch.float16)
    lab = torch.tensor([3, -1, 0, 4, -1, 1][:rows], dtype=torch.int32)
    g[:, -2:] = lab.view(torch.float16).reshape(rows, 2)          # the label's int32 bits in the last two fp16 columns (include/ovmr_hip.h)
    return {"gathered": g.to(dev), "C": c, "D": E, "n_ctx": N_CTX}


def _detail_ops(dev, b=6, c=C, k=2):
    z = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    return {"mo": _f("dmo", b, c).to(dev), "labels": _ints("dl", b, c).to(dev), "k": k, "counts": z(3 * c + 1), "hits": z(1), "class_hits": z(c),
            "cmat": z(c, c)}


BASE = {
    "set_weight": lambda dev: {"name": "text_projection", "tensor": _f("tp", W, E, scale=W ** -0.5).to(dev)},
    "encode_image": lambda dev: {"image": _f("img", B, 3, R, R).to(dev)},
    "encode_text_embedded": lambda dev: {"prompts": _f("pr", N, CTX, W, dtype=torch.float16, scale=0.02).to(dev),
                                         "index": torch.tensor([5, 4, 7], dtype=torch.int32).to(dev)},
    "encode_text_ids": lambda dev: {"ids": _ids(N).to(dev)},
    "encode_text_groups": lambda dev: {"groups": [{"ids": _ids(N).to(dev), "normalize": 1},
                                                  {"prompts": _f("gpr", 2, CTX, W, dtype=torch.float16, scale=0.02).to(dev),
                                                   "index": torch.tensor([6, 3], dtype=torch.int32).to(dev), "seq_len": 8}]},
    "encode_text_ensemble": lambda dev: {"ids": torch.stack([_ids(N, 1), _ids(N, 2)]).to(dev)},
    "embed_tokens": lambda dev: {"ids": _ids(N).to(dev)},
    "generate_tokens": lambda dev: {"feats": _unit("gf", CB * S).reshape(CB, S, E).to(dev)},
    "generate_tokens_ragged": lambda dev: {"feats": _unit("rf", 7).to(dev), "shots": [3, 1, 3]},
    "assemble_prompts": lambda dev: {"base": _f("ab", C, CTX, W, dtype=torch.float16, scale=0.02).to(dev), "labels": torch.tensor([4, 0, 2]).to(dev),
                                     "tokens": _f("at", CB, N_CTX, W).to(dev)},
    "xval_counts": lambda dev: {"feats": _unit("xf", 7).to(dev), "labels": _ints("xl", 7, C, torch.int32).to(dev), "clf": _unit("xc", C).to(dev),
                                "tp": torch.zeros(C, dtype=torch.int32, device=dev), "n_pred": torch.zeros(C, dtype=torch.int32, device=dev)},
    "fusion_weights": lambda dev: {"counts": _ints("fc", 6 * C, 5, torch.int32).reshape(3, 2, C).to(dev),
                                   "n_label": torch.full((C,), 4, dtype=torch.int32).to(dev), "tau": 10.0},
    "fused_logits": _head,
    "fused_logits_all": _head,
    "zeroshot_logits": lambda dev: {"feats": _unit("zf", B).to(dev), "text_feats": _unit("zt", C).to(dev)},
    "pack_rows": _packed,
    "unpack_rows": _gathered,
    "eval_counts": lambda dev: {"mo": _f("emo", 6, C).to(dev), "gt": _ints("egt", 6, C).to(dev)},
    "topk_rows": lambda dev: {"mo": _f("tmo", 6, C).to(dev), "k": 2, "labels": _ints("tl", 6, C).to(dev), "hits": torch.zeros(1, dtype=torch.int32, device=dev)},
    "eval_detail": _detail_ops,
    "preprocess_u8": lambda dev: {"u8": _ints("u8", 2 * R * R * 3, 256, torch.uint8).reshape(2, R, R, 3).to(dev)},
}

Case = namedtuple("Case", "wrapper name build arg")      # build(dev) -> the operands; arg: the argument a violation is about


def _with(wrapper, **changes):
    """The base operands with some replaced: a value f(plain host tensor of that operand, dev), or a constant."""
    def build(dev):
        ops = BASE[wrapper](dev)
        host = BASE[wrapper]("cpu")
        for k, f in changes.items():
            ops[k] = f(host.get(k), dev) if callable(f) else f
        return ops
    return build


def _laid(wrapper, operand, layout):
    return Case(wrapper, f"{operand} {layout}", _with(wrapper, **{operand: LAYOUTS[layout]}), None)


def _const(f):
    """An operand built from the device alone."""
    return lambda _x, dev: f(dev)


SENTINEL = 0x5A                                           # every byte of a buffer a caller's `out` is a slice of


def _sentinel(shape, dtype, dev):
    """A buffer of `dtype` whose every byte is the sentinel (shape: the last extent in bytes); `.whole` is the same memory as uint8."""
    whole = torch.full(shape, SENTINEL, dtype=torch.uint8, device=dev)
    out = whole.view(dtype)
    out.whole = whole
    return out


def _out_slice(shape, dtype, rows, dim=0):
    """out = big[r0:r1] (or big[:, r0:r1]) of a larger buffer filled with the sentinel; out.whole is that buffer, as uint8."""
    item = torch.empty((), dtype=dtype).element_size()

    def make(_x, dev):
        big = _sentinel(tuple(shape[:-1]) + (shape[-1] * item,), dtype, dev)
        out = big[rows] if dim == 0 else big[:, rows]
        out.whole = big.whole
        return out
    return make


def _accepted():
    A = [Case(w, "plain", BASE[w], None) for w in BASE]
    add = lambda wrapper, name, **ch: A.append(Case(wrapper, name, _with(wrapper, **ch), None))
    lay = lambda wrapper, operand, *layouts: A.extend(_laid(wrapper, operand, l) for l in layouts)

    lay("set_weight", "tensor", "numpy", "host", "fp16", "fp64", "transposed", "offset")
    lay("encode_image", "image", "numpy", "host", "fp16", "fp64", "channels_last", "hw_transposed", "offset", "expanded")
    add("encode_image", "image uint8", image=lambda x, dev: (x * 40 + 128).clamp(0, 255).to(torch.uint8).to(dev))
    add("encode_image", "image fp16 offset", image=lambda x, dev: offset(x.half(), dev))
    add("encode_image", "one image", image=lambda x, dev: x[:1].to(dev))
    add("encode_image", "7 images, not normalised", image=lambda x, dev: torch.cat([x, x, x[:1]]).to(dev), normalize=False)
    add("encode_image", "out", out=_const(lambda dev: _sentinel((B, E * 2), torch.float16, dev)))
    add("encode_image", "out row slice", out=_out_slice((7, E), torch.float16, slice(2, 2 + B)))

    lay("encode_text_embedded", "prompts", "numpy", "host", "fp32", "offset", "expanded")
    lay("encode_text_embedded", "index", "numpy", "host", "int64", "offset")
    add("encode_text_embedded", "seq_len 8, normalize 2", seq_len=8, normalize=2)
    add("encode_text_embedded", "prompts stored [ctx, N, W]", prompts=lambda x, dev: transposed(x, dev, 0, 1))

    lay("encode_text_ids", "ids", "numpy", "host", "int32", "offset", "transposed", "expanded")
    add("encode_text_ids", "seq_len 8, normalize 1", seq_len=8, normalize=1)
    add("encode_text_ids", "7 prompts", ids=_const(lambda dev: _ids(7).to(dev)))

    add("encode_text_groups", "ids int32, prompts offset", groups=lambda g, dev: [
        dict(BASE["encode_text_groups"](dev)["groups"][0], ids=LAYOUTS["int32"](g[0]["ids"], dev)),
        dict(BASE["encode_text_groups"](dev)["groups"][1], prompts=offset(g[1]["prompts"], dev))])
    add("encode_text_groups", "host ids, numpy index", groups=lambda g, dev: [
        dict(BASE["encode_text_groups"](dev)["groups"][0], ids=g[0]["ids"]),
        dict(BASE["encode_text_groups"](dev)["groups"][1], index=g[1]["index"].numpy())])
    add("encode_text_groups", "ids transposed, index int64 offset", groups=lambda g, dev: [
        dict(BASE["encode_text_groups"](dev)["groups"][0], ids=transposed(g[0]["ids"], dev)),
        dict(BASE["encode_text_groups"](dev)["groups"][1], index=offset(g[1]["index"].long(), dev))])

    lay("encode_text_ensemble", "ids", "numpy", "host", "int32", "offset")
    add("encode_text_ensemble", "ids stored [C, T, ctx]", ids=lambda x, dev: transposed(x, dev, 0, 1))
    add("encode_text_ensemble", "seq_lens", seq_lens=[8, 8])
    add("encode_text_ensemble", "no class", ids=lambda x, dev: x[:, :0].to(dev))                      # C == 0 returns 0

    lay("embed_tokens", "ids", "numpy", "host", "int32", "offset", "transposed", "expanded")
    add("embed_tokens", "ids [2, 5]", ids=lambda x, dev: x[:2, :5].to(dev))
    add("embed_tokens", "the template row", ids=_const(lambda dev: torch.from_numpy(synth.template_token_ids(CTX)).to(dev)))

    lay("generate_tokens", "feats", "numpy", "host", "fp32", "offset", "expanded")
    add("generate_tokens", "feats stored [S, Cb, E]", feats=lambda x, dev: transposed(x, dev, 0, 1))
    add("generate_tokens", "one shot", feats=lambda x, dev: x[:, :1].to(dev))

    lay("generate_tokens_ragged", "feats", "numpy", "host", "fp32", "offset", "transposed")
    add("generate_tokens_ragged", "shots numpy", shots=np.asarray([3, 1, 3], dtype=np.int64))
    add("generate_tokens_ragged", "shots host tensor", shots=torch.tensor([3, 1, 3], dtype=torch.int32))
    add("generate_tokens_ragged", "no class", feats=lambda x, dev: x[:0].to(dev), shots=[])            # Cb == 0 returns 0

    lay("assemble_prompts", "base", "numpy", "host", "fp32", "offset")
    lay("assemble_prompts", "labels", "numpy", "host", "int32", "offset")
    lay("assemble_prompts", "tokens", "numpy", "host", "fp16", "offset", "transposed")
    add("assemble_prompts", "no labels, one template row", labels=None, base=lambda x, dev: x[:1].to(dev))
    add("assemble_prompts", "tokens expanded", tokens=expanded)

    lay("xval_counts", "feats", "numpy", "host", "fp32", "offset", "transposed")
    lay("xval_counts", "labels", "numpy", "host", "int64", "offset")
    lay("xval_counts", "clf", "host", "fp32", "transposed")
    add("xval_counts", "labels expanded view (one class, its rows)", labels=lambda x, dev: x[:1].to(dev).unsqueeze(1).expand(-1, 7).reshape(-1))
    add("xval_counts", "tp, n_pred rows of a [3, 2, C] tensor",
        tp=_const(lambda dev: torch.zeros((3, 2, C), dtype=torch.int32, device=dev)[1, 0]),
        n_pred=_const(lambda dev: torch.zeros((3, 2, C), dtype=torch.int32, device=dev)[1, 1]))
    add("xval_counts", "tp longer than C", tp=_const(lambda dev: torch.zeros(C + 3, dtype=torch.int32, device=dev)))

    lay("fusion_weights", "counts", "numpy", "host", "int64", "offset")
    lay("fusion_weights", "n_label", "numpy", "host", "int64", "expanded")
    add("fusion_weights", "counts stored [C, 2, 3]", counts=lambda x, dev: transposed(x, dev, 0, 2))

    for w in ("fused_logits", "fused_logits_all"):
        lay(w, "feats", "numpy", "host", "fp32", "offset", "transposed", "expanded")
        lay(w, "mm", "host", "fp32", "offset")
        lay(w, "t", "transposed")
        lay(w, "w", "numpy", "fp64", "offset", "transposed")
    for mode, keep in (("text", "t"), ("vision", "v"), ("multimodal", "mm")):
        add("fused_logits", f"mode {mode}, the other classifiers None", mode=mode, w=None, **{k: None for k in ("mm", "v", "t") if k != keep})
    add("fused_logits", "out", out=_const(lambda dev: _sentinel((B, C * 4), torch.float32, dev)))
    add("fused_logits", "out row slice", out=_out_slice((7, C), torch.float32, slice(1, 1 + B)))
    add("fused_logits_all", "out", out=_const(lambda dev: _sentinel((4, B, C * 4), torch.float32, dev)))
    add("fused_logits_all", "out rows of [4, Btot, C]", out=_out_slice((4, 7, C), torch.float32, slice(2, 2 + B), dim=1))
    add("fused_logits_all", "empty batch", feats=lambda x, dev: x[:0].to(dev))                         # B == 0 returns 0
    add("fused_logits_all", "empty batch into rows of [4, Btot, C]", feats=lambda x, dev: x[:0].to(dev),
        out=_out_slice((4, 7, C), torch.float32, slice(2, 2), dim=1))

    lay("zeroshot_logits", "feats", "numpy", "host", "fp32", "offset", "transposed", "expanded")
    lay("zeroshot_logits", "text_feats", "host", "fp32", "offset", "transposed")
    add("zeroshot_logits", "out", out=_const(lambda dev: _sentinel((B, C * 2), torch.float16, dev)))
    add("zeroshot_logits", "out row slice", out=_out_slice((7, C), torch.float16, slice(4, 4 + B)))

    lay("pack_rows", "labels", "numpy", "host", "int32", "offset")
    add("pack_rows", "mm a row slice", mm=offset)
    add("pack_rows", "as many rows as the bound", bound=3)
    add("pack_rows", "no row", labels=lambda x, dev: x[:0].to(dev))

    lay("unpack_rows", "gathered", "numpy", "host", "offset", "transposed")

    lay("eval_counts", "mo", "fp16", "fp64", "offset", "transposed")
    add("eval_counts", "mo columns of a wider matrix", mo=lambda x, dev: torch.cat([x, x], 1).to(dev)[:, :C])
    lay("eval_counts", "gt", "host", "int32", "offset")
    lay("topk_rows", "mo", "fp16", "offset", "transposed", "expanded")
    add("topk_rows", "mo columns of a wider matrix", mo=lambda x, dev: torch.cat([x, x], 1).to(dev)[:, :C])
    add("topk_rows", "no labels", labels=None, hits=None)
    add("topk_rows", "empty batch", mo=lambda x, dev: x[:0].to(dev), labels=lambda x, dev: x[:0].to(dev))      # B == 0 returns 0
    lay("eval_detail", "mo", "fp16", "offset")
    add("eval_detail", "mo columns of a wider matrix", mo=lambda x, dev: torch.cat([x, x], 1).to(dev)[:, :C])
    add("eval_detail", "counts only", hits=None, class_hits=None, cmat=None)
    add("eval_detail", "empty batch", mo=lambda x, dev: x[:0].to(dev), labels=lambda x, dev: x[:0].to(dev))    # B == 0 returns 0
    lay("preprocess_u8", "u8", "offset")
    add("preprocess_u8", "out", out=_const(lambda dev: _sentinel((2, 3, R, R * 2), torch.float16, dev)))
    add("preprocess_u8", "out slice, no normalisation", mean=None, out=_out_slice((5, 3, R, R), torch.float16, slice(1, 3)))
    return A


def _violations():
    V = []
    bad = lambda wrapper, arg, name, **ch: V.append(Case(wrapper, name, _with(wrapper, **ch), arg))
    cut = lambda dim, n: (lambda x, dev: x.narrow(dim, 0, n).to(dev))                    # a dimension too short
    pad = lambda dim: (lambda x, dev: torch.cat([x, x.narrow(dim, 0, 1)], dim).to(dev))  # one too long
    meta = lambda shape, dtype: _const(lambda dev: torch.empty(shape, dtype=dtype, device="meta"))   # stands for "not on the engine's device"
    dev_t = lambda shape, dtype: _const(lambda dev: torch.zeros(shape, dtype=dtype, device=dev))

    bad("set_weight", "tensor", "a list", tensor=[[1.0, 2.0]])
    bad("set_weight", "tensor", "complex", tensor=lambda x, dev: x.to(torch.complex64).to(dev))

    bad("encode_image", "image", "resolution 8", image=_const(lambda dev: torch.zeros(2, 3, 8, 8, device=dev)))      # (reproduced on the parent commit)
    bad("encode_image", "image", "resolution 40", image=_const(lambda dev: torch.zeros(2, 3, 40, 40, device=dev)))
    bad("encode_image", "image", "not square", image=cut(3, R - 8))
    bad("encode_image", "image", "one channel", image=cut(1, 1))
    bad("encode_image", "image", "four channels", image=pad(1))
    bad("encode_image", "image", "channels last by shape", image=lambda x, dev: x.permute(0, 2, 3, 1).to(dev))
    bad("encode_image", "image", "three dimensions", image=lambda x, dev: x[0].to(dev))
    bad("encode_image", "image", "numpy of resolution 8", image=np.zeros((2, 3, 8, 8), dtype=np.float32))
    bad("encode_image", "out", "out of another batch", out=dev_t((B + 1, E), torch.float16))
    bad("encode_image", "out", "out of another width", out=dev_t((B, E // 2), torch.float16))
    bad("encode_image", "out", "out fp32", out=dev_t((B, E), torch.float32))
    bad("encode_image", "out", "out on another device", out=meta((B, E), torch.float16))
    bad("encode_image", "out", "out strided", out=_const(lambda dev: torch.zeros((B, 2 * E), dtype=torch.float16, device=dev)[:, ::2]))
    bad("encode_image", "out", "out a numpy array", out=np.zeros((B, E), dtype=np.float16))

    for w in ("encode_text_ids", "embed_tokens"):
        bad(w, "ids", "a token id of vocab_size (host)", ids=lambda x, dev: x.clone().index_put_((torch.tensor(1), torch.tensor(2)), torch.tensor(TINY.vocab)))
        bad(w, "ids", "a negative token id (numpy)", ids=lambda x, dev: np.where(x.numpy() == 0, -1, x.numpy()))
    bad("encode_text_ids", "ids", "ids [3, 5]", ids=cut(1, 5))                                                          # (reproduced on the parent commit)
    bad("encode_text_ids", "ids", "ids [3, 78]", ids=pad(1))
    bad("encode_text_ids", "ids", "ids flat", ids=lambda x, dev: x.reshape(-1).to(dev))
    bad("encode_text_ids", "ids", "ids [1, 3, 77]", ids=lambda x, dev: x[None].to(dev))
    bad("embed_tokens", "ids", "ids flat", ids=lambda x, dev: x.reshape(-1).to(dev))
    bad("embed_tokens", "ids", "ids three-dimensional", ids=lambda x, dev: x[None].to(dev))

    bad("encode_text_embedded", "prompts", "prompts of 5 positions", prompts=cut(1, 5))
    bad("encode_text_embedded", "prompts", "prompts of width 64", prompts=cut(2, 64))
    bad("encode_text_embedded", "prompts", "prompts of width 129", prompts=pad(2))
    bad("encode_text_embedded", "prompts", "prompts two-dimensional", prompts=lambda x, dev: x[0].to(dev))
    bad("encode_text_embedded", "index", "index shorter", index=cut(0, N - 1))
    bad("encode_text_embedded", "index", "index longer", index=pad(0))
    bad("encode_text_embedded", "index", "index [N, 1]", index=lambda x, dev: x[:, None].to(dev))

    grp = lambda k, key, f: (lambda g, dev: [dict(h, **({key: f(g[k][key], dev)} if j == k else {}))
                                             for j, h in enumerate(BASE["encode_text_groups"](dev)["groups"])])
    bad("encode_text_groups", "ids", "ids [3, 5] in group 0", groups=grp(0, "ids", cut(1, 5)))
    bad("encode_text_groups", "prompts", "prompts of width 64 in group 1", groups=grp(1, "prompts", cut(2, 64)))
    bad("encode_text_groups", "prompts", "prompts of 76 positions in group 1", groups=grp(1, "prompts", cut(1, CTX - 1)))
    bad("encode_text_groups", "index", "index longer in group 1", groups=grp(1, "index", pad(0)))
    bad("encode_text_groups", "ids", "a token id of vocab_size in group 0 (host)",
        groups=grp(0, "ids", lambda x, dev: x.clone().index_put_((torch.tensor(0), torch.tensor(1)), torch.tensor(TINY.vocab))))

    bad("encode_text_ensemble", "ids", "ids [2, 3, 5]", ids=cut(2, 5))
    bad("encode_text_ensemble", "ids", "ids [3, 77]", ids=lambda x, dev: x[0].to(dev))
    bad("encode_text_ensemble", "seq_lens", "three seq_lens for two templates", seq_lens=[8, 8, 8])
    bad("encode_text_ensemble", "seq_lens", "one seq_len for two templates", seq_lens=[8])
    bad("encode_text_ensemble", "ids", "a token id of vocab_size (host)", ids=lambda x, dev: x.clone().index_put_(
        (torch.tensor(1), torch.tensor(0), torch.tensor(1)), torch.tensor(TINY.vocab)))

    bad("generate_tokens", "feats", "feats of width 64", feats=cut(2, 64))
    bad("generate_tokens", "feats", "feats packed [R, E]", feats=lambda x, dev: x.flatten(0, 1).to(dev))
    bad("generate_tokens_ragged", "feats", "feats of width 64", feats=cut(1, 64))
    bad("generate_tokens_ragged", "feats", "feats [Cb, S, E]", feats=lambda x, dev: x[:6].reshape(2, 3, E).to(dev))

    bad("assemble_prompts", "base", "base of 76 positions", base=cut(1, CTX - 1))
    bad("assemble_prompts", "base", "base of width 64", base=cut(2, 64))
    bad("assemble_prompts", "base", "base two-dimensional", base=lambda x, dev: x[0].to(dev))
    bad("assemble_prompts", "base", "base without a row", base=cut(0, 0))
    bad("assemble_prompts", "tokens", "tokens of 3 rows per class", tokens=pad(1))
    bad("assemble_prompts", "tokens", "tokens of one row per class", tokens=cut(1, 1))
    bad("assemble_prompts", "tokens", "tokens of width 64", tokens=cut(2, 64))
    bad("assemble_prompts", "tokens", "tokens flattened [Cb, n_ctx * W]", tokens=lambda x, dev: x.flatten(1).to(dev))
    bad("assemble_prompts", "labels", "labels longer", labels=pad(0))
    bad("assemble_prompts", "labels", "labels shorter", labels=cut(0, CB - 1))
    bad("assemble_prompts", "labels", "a label beyond base's rows (host)", labels=torch.tensor([4, C, 2]))
    bad("assemble_prompts", "labels", "a negative label (host)", labels=torch.tensor([4, -1, 2]))

    bad("xval_counts", "feats", "feats of width 64", feats=cut(1, 64))
    bad("xval_counts", "labels", "labels shorter", labels=cut(0, 6))
    bad("xval_counts", "labels", "labels longer", labels=pad(0))
    bad("xval_counts", "clf", "clf of width 129", clf=pad(1))
    bad("xval_counts", "tp", "tp shorter than C", tp=dev_t((C - 1,), torch.int32))
    bad("xval_counts", "n_pred", "n_pred shorter than C", n_pred=dev_t((C - 1,), torch.int32))
    bad("xval_counts", "tp", "tp int64", tp=dev_t((C,), torch.int64))
    bad("xval_counts", "n_pred", "n_pred int64", n_pred=dev_t((C,), torch.int64))
    bad("xval_counts", "tp", "tp strided", tp=_const(lambda dev: torch.zeros(2 * C, dtype=torch.int32, device=dev)[::2]))
    bad("xval_counts", "n_pred", "n_pred on another device", n_pred=meta((C,), torch.int32))

    bad("fusion_weights", "counts", "counts [3, 2, C - 1]", counts=cut(2, C - 1))
    bad("fusion_weights", "counts", "counts [2, 2, C]", counts=cut(0, 2))
    bad("fusion_weights", "counts", "counts [3, C]", counts=lambda x, dev: x[:, 0].to(dev))
    bad("fusion_weights", "counts", "counts flat", counts=lambda x, dev: x.reshape(-1).to(dev))
    bad("fusion_weights", "n_label", "n_label [C, 1]", n_label=lambda x, dev: x[:, None].to(dev))

    for w in ("fused_logits", "fused_logits_all"):
        bad(w, "feats", "feats of width 64", feats=cut(1, 64))
        bad(w, "feats", "feats three-dimensional", feats=lambda x, dev: x[None].to(dev))
        bad(w, "mm", "mm of width 129", mm=pad(1))
        bad(w, "v", "v with a row less", v=cut(0, C - 1))
        bad(w, "t", "t with a row more", t=pad(0))
        bad(w, "w", "w [C, 2]", w=cut(1, 2))
        bad(w, "w", "w [C - 1, 3]", w=cut(0, C - 1))
        bad(w, "w", "w [3, C]", w=lambda x, dev: x.t().contiguous().to(dev))
    bad("fused_logits", "mm / v / t", "no classifier at all", mm=None, v=None, t=None, mode="text")
    bad("fused_logits", "out", "out [B, C + 1]", out=dev_t((B, C + 1), torch.float32))
    bad("fused_logits", "out", "out fp16", out=dev_t((B, C), torch.float16))
    bad("fused_logits", "out", "out on another device", out=meta((B, C), torch.float32))
    bad("fused_logits", "out", "out columns of a wider matrix", out=_const(lambda dev: torch.zeros((B, C + 2), device=dev)[:, :C]))
    bad("fused_logits_all", "t", "t missing", t=None)
    bad("fused_logits_all", "w", "w missing", w=None)
    bad("fused_logits_all", "out", "out [B, C]", out=dev_t((B, C), torch.float32))
    bad("fused_logits_all", "out", "out [3, B, C]", out=dev_t((3, B, C), torch.float32))
    bad("fused_logits_all", "out", "out fp16", out=dev_t((4, B, C), torch.float16))
    bad("fused_logits_all", "out", "out on another device", out=meta((4, B, C), torch.float32))
    bad("fused_logits_all", "out", "out columns of a wider tensor", out=_const(lambda dev: torch.zeros((4, B, C + 2), device=dev)[:, :, :C]))
    bad("fused_logits_all", "out", "out with overlapping planes", out=_const(lambda dev: torch.zeros((1, B, C), device=dev).expand(4, -1, -1)))

    bad("zeroshot_logits", "feats", "feats of width 64", feats=cut(1, 64))
    bad("zeroshot_logits", "text_feats", "text_feats of width 129", text_feats=pad(1))
    bad("zeroshot_logits", "text_feats", "text_feats flat", text_feats=lambda x, dev: x.reshape(-1).to(dev))
    bad("zeroshot_logits", "out", "out [B + 1, C]", out=dev_t((B + 1, C), torch.float16))
    bad("zeroshot_logits", "out", "out fp32", out=dev_t((B, C), torch.float32))
    bad("zeroshot_logits", "out", "out on another device", out=meta((B, C), torch.float16))
    bad("zeroshot_logits", "out", "out transposed", out=_const(lambda dev: torch.zeros((C, B), dtype=torch.float16, device=dev).t()))

    bad("pack_rows", "v", "v with a row less", v=cut(0, C - 1))
    bad("pack_rows", "t", "t fp32", t=LAYOUTS["fp32"])
    bad("pack_rows", "mm", "mm strided", mm=lambda x, dev: transposed(x, dev))
    bad("pack_rows", "mm", "mm on another device", mm=meta((C, E), torch.float16))
    bad("pack_rows", "tokens", "tokens of another width", tokens=cut(2, 64))
    bad("pack_rows", "tokens", "tokens flattened", tokens=lambda x, dev: x.flatten(1).to(dev))
    bad("pack_rows", "labels", "labels [n, 1]", labels=lambda x, dev: x[:, None].to(dev))
    bad("unpack_rows", "gathered", "gathered a column short", gathered=cut(1, (3 + N_CTX) * E + 1))
    bad("unpack_rows", "gathered", "gathered without the label columns", gathered=cut(1, (3 + N_CTX) * E))
    bad("unpack_rows", "gathered", "gathered flat", gathered=lambda x, dev: x.reshape(-1).to(dev))
    bad("unpack_rows", "gathered", "n_ctx of another model", n_ctx=N_CTX + 1)

    # the evaluator's entry points and the loader's take device tensors as they are: a host tensor is itself a violation
    cpu = lambda x, dev: x
    bad("eval_counts", "mo", "mo of C + 1 columns", mo=pad(1))
    bad("eval_counts", "gt", "gt shorter", gt=cut(0, 5))
    bad("topk_rows", "mo", "mo on the host", mo=cpu)
    bad("topk_rows", "mo", "mo flat", mo=lambda x, dev: x.reshape(-1))
    bad("topk_rows", "mo", "mo fp64", mo=lambda x, dev: x.double())
    bad("eval_detail", "mo", "mo on the host", mo=cpu)
    bad("eval_detail", "mo", "mo three-dimensional", mo=lambda x, dev: x[None])
    bad("preprocess_u8", "u8", "u8 on the host", u8=cpu)
    bad("preprocess_u8", "u8", "u8 float", u8=lambda x, dev: x.float())
    # ... and these get past the device check only with tensors on a GPU: the CPU test lifts that ONE condition for them (NEEDS_DEVICE)
    bad("topk_rows", "labels", "labels shorter", labels=cut(0, 5))
    bad("topk_rows", "labels", "labels int32", labels=LAYOUTS["int32"])
    bad("topk_rows", "hits", "hits int64", hits=dev_t((1,), torch.int64))
    bad("topk_rows", "hits", "hits empty", hits=dev_t((0,), torch.int32))
    bad("eval_detail", "mo", "mo with a column stride", mo=lambda x, dev: transposed(x, dev))
    bad("eval_detail", "mo", "mo an expanded row", mo=expanded)
    bad("eval_detail", "labels", "labels longer", labels=pad(0))
    bad("eval_detail", "labels", "labels int32", labels=LAYOUTS["int32"])
    bad("eval_detail", "counts", "counts without the last slot", counts=dev_t((3 * C,), torch.int32))
    bad("eval_detail", "class_hits", "class_hits shorter", class_hits=dev_t((C - 1,), torch.int32))
    bad("eval_detail", "cmat", "cmat [C, C - 1]", cmat=dev_t((C, C - 1), torch.int32))
    bad("eval_detail", "cmat", "cmat int64", cmat=dev_t((C, C), torch.int64))
    bad("preprocess_u8", "u8", "frames not square", u8=cut(2, R - 8))
    bad("preprocess_u8", "u8", "frames of side 36", u8=_const(lambda dev: torch.zeros((2, 36, 36, 3), dtype=torch.uint8, device=dev)))
    bad("preprocess_u8", "u8", "four channels", u8=pad(3))
    bad("preprocess_u8", "u8", "channels first", u8=lambda x, dev: x.permute(0, 3, 1, 2).contiguous().to(dev))
    bad("preprocess_u8", "u8", "u8 strided", u8=lambda x, dev: transposed(x, dev, 1, 2))
    bad("preprocess_u8", "out", "out of another batch", out=dev_t((3, 3, R, R), torch.float16))
    bad("preprocess_u8", "out", "out channels last by shape", out=dev_t((2, R, R, 3), torch.float16))
    bad("preprocess_u8", "out", "out fp32", out=dev_t((2, 3, R, R), torch.float32))
    bad("preprocess_u8", "out", "out strided", out=_const(lambda dev: torch.zeros((2, 3, R, 2 * R), dtype=torch.float16, device=dev)[..., ::2]))
    return V


ACCEPTED = _accepted()
VIOLATIONS = _violations()


NEEDS_DEVICE = lambda c: c.wrapper in DEVICE_ONLY and c.wrapper != "eval_counts" and "on the host" not in c.name


def case_id(c):
    return f"{c.wrapper}: {c.name}"
