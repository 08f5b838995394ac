"""The launch sequences of ovmr_api.hip -- ovmr_encode_image, run_block_f16, ln_linear, run_text_groups, run_text_group_chunked,
generate_tokens, run_block_f32 and the derived weight layouts of ovmr_finalize -- replayed kernel by kernel.  Plain torch, importable
without a GPU: shared by test_engine_replay_cpu.py and test_hip_engine_replay.py.

The method.  Every kernel is held to exact values by a test of its own; what strings the kernels together was held to 1e-3 in cosine
against the oracle.  The debug hooks launch the same kernels as the engine through the same routing functions, so the engine's
output on an input is, bit for bit, what comes out when the same launches are made one by one through the hooks in the order
clip/model.py prescribes.  Three links then hold the whole path, none of them with a tolerance on the GPU:

    wiring  == reference model      the `torch` backend against the oracle, on the CPU (test_engine_replay_cpu.py);
    engine  == wiring over kernels  the engine against the `hooks` backend, as bit patterns (test_hip_engine_replay.py);
    kernels == exact values         the kernel tests (test_hip_*_exact.py).

Each of the three paths -- image_tower, text_tower, generator -- is stated ONCE here, as a sequence of steps over named buffers.  A
step is one hook call: `be.step("gemm", A=..., ...)`; an operand is a buffer name or Ref(name, element offset).  A backend executes it:

    Planner   records the steps and executes nothing: plan(case), the list of launches with shapes, strides, variant and the kernel
              each takes (gemm_exact.route / attn_exact.route, the restatements the library's exported routes are held to);
    Torch     every step as plain torch on the CPU in one dtype (float64: no rounding anywhere); it exists only to prove the wiring;
    Hooks     launches through the library (test_hip_engine_replay.py).

The two copies without arithmetic -- cat([cls_token, feats.float()]) in front of the aggregator and the first n_ctx rows behind it --
are steps of their own ("agg_input", "agg_output") that every backend runs in torch.

A mutation is a planted wiring slip: a name in MUTATIONS that the path functions consult where the wire is (`mut == ...`), setting
be.hit where that step runs.  Unmutated, be.hit stays False.

What the replay pins, and why:

  * last_q_cls = 0 where a launch sequence holds at least 256 images.  The strided hook takes the CLS-row Q launch's statistics from a
    row-statistics pass, the engine from c_proj's epilogue; the two need not agree in the last bit.
    test_last_block_projects_q_for_the_cls_rows_only ties 1 to 0 bit for bit, so nothing is lost.
  * The engine's ONE launch of attn_f16_short over up to four groups is replayed as one launch per group: per (sequence, head) the
    arithmetic is the same by construction; a difference is a finding in AttnShortGroups' indexing.
  * A text pass that does not fit the workspace (ovmr_encode_text_groups falling back to group-by-group, ovmr_encode_text_ensemble
    splitting the classes) is not in the table: the head's reserve alone is 192 MiB, text_rows_fit asserts the cases stay under it.
  * agg_max_len is set after ovmr_finalize (as every option of a case), so the aggregator's row capacity is max_classes * (n_ctx + 32).
"""
import ctypes
import dataclasses
import functools
import zlib
from typing import NamedTuple

import torch
import torch.nn.functional as F

import attn_exact as AX
import gemm_exact as G
from ovmr_amd import synth

EPI_NONE, EPI_BIAS, EPI_BIAS_QGELU, EPI_BIAS_RES, EPI_PATCH = G.EPI_NONE, G.EPI_BIAS, G.EPI_BIAS_QGELU, G.EPI_BIAS_RES, G.EPI_PATCH
N_CU = 256                              # an MI355X; the planner's default (the GPU test plans with the device's own count)
N_CTX = 2
EOT, SOT = 511, 510                     # the specs below have 512 token ids: EOT is the largest (clip/model.py:831)
OPTION_DEFAULTS = {"gemm": 8, "attn": 3, "gelu_exact": 0, "ln_fold": 1, "fuse_im2col": 1, "last_q_cls": 1, "enc_chunk": 0,
                   "agg_max_len": 128}


def _spec(base, name, vision_layers=None, transformer_layers=None):
    s = synth.SPECS[base]
    return dataclasses.replace(s, name=name, vocab_size=512,
                               vision_layers=s.vision_layers if vision_layers is None else vision_layers,
                               transformer_layers=s.transformer_layers if transformer_layers is None else transformer_layers)


# The geometries of synth.SPECS with 512 token ids (the token table is the one weight whose size no step depends on) and, for
# localisation, with one block and with two: the first of the two to fail names the block.
SPECS = {
    "tiny": _spec("tiny", "tiny"), "tiny1": _spec("tiny", "tiny1", 1, 1),
    "small": _spec("small", "small"), "small1": _spec("small", "small1", 1, 1), "small2": _spec("small", "small2", 2, 2),
    "b16x2": _spec("ViT-B/16", "b16x2", 2, 1), "b16x1": _spec("ViT-B/16", "b16x1", 1, 1),
    "head768": _spec("head768", "head768"), "head768x1": _spec("head768", "head768x1", 1, 1),
}


class Ref(NamedTuple):
    name: str
    off: int = 0                        # in elements


def ref(x, off=0):
    return x if isinstance(x, Ref) else Ref(x, off)


class Case(NamedTuple):
    name: str
    path: str                           # "image" | "text" | "gen"
    spec: str                           # key of SPECS
    opts: dict                          # options set after ovmr_finalize (OPTION_DEFAULTS for the rest)
    reserve: tuple                      # ovmr_finalize(max_images, max_prompts, max_classes)
    entry: str                          # the engine's entry point
    args: dict


def options(case):
    o = dict(OPTION_DEFAULTS)
    o.update(case.opts)
    return o


# ---- the fold decision and the launch sequences of a batch: ovmr_api.hip restated (the GPU test holds the second to ovmr_encode_plan) ----

def can_fold(o, M, W):
    """can_fold_ln: the statistics come in 256-column slots, from the tile kernel alone, so not where the N = W launches take the split-K
    kernel (gemm_f16_latency_bound: gemm_exact.route says "s64" for out_proj under the engine's variant 8)."""
    latency_bound = o["gemm"] == 8 and G.route(8, M, W, W, EPI_BIAS_RES)[0] == "s64"
    return bool(o["ln_fold"]) and M >= 256 and W % 256 == 0 and W // 256 <= 64 and not latency_bound


def _pick_encode_chunk(max_images, L, W, n_cu):
    nw = max(1, W // 256)
    tiles = lambda b: (b * L + 255) // 256
    rounds = lambda wg: (wg + n_cu - 1) // n_cu
    if n_cu < 1 or tiles(max_images) * nw < 2 * n_cu:
        return max_images
    cost = lambda b: 5 * rounds(tiles(b) * nw) + rounds(3 * tiles(b) * nw) + rounds(4 * tiles(b) * nw)
    top = min(max_images, max(1, 600 * 256 // L))
    best, best_rate = top, top / cost(top)
    for b in range(top - 1, max(1, top * 3 // 4) - 1, -1):
        if b / cost(b) > best_rate * 1.002:
            best_rate, best = b / cost(b), b
    return best


def encode_plan(case, n_cu=N_CU):
    """Images per launch sequence of the case's ovmr_encode_image call (encode_plan, set_enc_chunk and the fold slack of ovmr_finalize)."""
    s, o = SPECS[case.spec], options(case)
    L, W, B, max_images = s.vision_tokens, s.vision_width, case.args["B"], case.reserve[0]
    nw = max(1, W // 256)
    big = (max_images * L + 255) // 256 * nw >= 2 * n_cu
    enc_fold = min(n_cu * 256 // (nw * L), max_images // 4) if big else 0
    img_cap = max_images + enc_fold
    enc_chunk = min(o["enc_chunk"], max_images) if o["enc_chunk"] > 0 else _pick_encode_chunk(max_images, L, W, n_cu)
    chunk = enc_chunk if o["enc_chunk"] > 0 or (B > max_images and enc_chunk > 0) else max_images
    out, b0 = [], 0
    while b0 < B:
        Bc = min(chunk, B - b0)
        left = B - b0 - Bc
        if 0 < left <= enc_fold and Bc + left <= img_cap:
            Bc += left
        out.append(Bc)
        b0 += Bc
    return out


def text_rows_fit(M, N, W):
    """text_ws(M, N) stays under the head's 192 MiB of logits (HeadWs), the floor of every workspace: one pass, whatever the reserve."""
    return (M * W * 9 + N * W) * 2 + N * 4 + M * ((W + 255) // 256) * 8 + 8 * 256 <= 192 << 20


# ---- backends -------------------------------------------------------------------------------------------------------------------

def _show(v):
    return f"{v.name}+{v.off}" if isinstance(v, Ref) and v.off else v.name if isinstance(v, Ref) else v


class Backend:
    """The steps a path makes; subclasses execute them.  plan: one dict per step -- the hook, its scalar arguments, its operands as
    "name+offset", and for the fp16 GEMM and attention launches the kernel the route sends them to."""

    def __init__(self, n_cu=N_CU):
        self.n_cu, self.plan, self.hit, self.rounding_only = n_cu, [], False, False

    def step(self, hook, **kw):
        rec = {"hook": hook}
        rec.update({k: _show(v) for k, v in kw.items() if not isinstance(v, (list, tuple))})
        if hook == "gemm" and not kw["f32"]:
            rec["route"] = G.route(kw["variant"], kw["M"], kw["N"], kw["K"], kw["epi"], kw["ldc"], kw["ldc"], stats=kw.get("stats") is not None)
        elif hook == "gemm_patches":
            rec["route"] = G.route(kw["variant"], kw["B"] * (kw["R"] >> 4) ** 2, kw["N"], 768, EPI_PATCH, kw["N"], im2col=kw["R"])
        elif hook == "gemm_strided":
            rec["route"] = G.route(kw["variant"], kw["M"], kw["N"], kw["K"], kw["epi"], kw["ldc"], kw["ldres"])
        elif hook == "lnfold":
            M, D, N2 = kw["M"], kw["D"], kw["N2"]
            if kw["A1"] is not None:
                rec["route1"] = G.route(kw["variant"], M, D, kw["K1"], EPI_BIAS_RES, D, D, stats=True)
            rec["route"] = G.route(kw["variant"], M, N2, D, G.EPI_LN_BIAS_QGELU if kw["qgelu"] else G.EPI_LN_BIAS, N2)
        elif hook in ("attention", "attention_q") and not kw.get("f32"):
            rec["route"] = AX.route(kw["variant"], kw["L"], kw.get("Lq", kw["L"]), kw["causal"])
        self.plan.append(rec)
        getattr(self, hook)(**kw)

    def alloc(self, name, elems, kind="f16"):
        pass


class Planner(Backend):
    def __getattr__(self, hook):
        return lambda **kw: None


def _gelu(x):
    return x * torch.sigmoid(1.702 * x)


def _unfold(img, P, Kpad):
    B, _, R, _ = img.shape
    g, K = R // P, 3 * P * P
    out = torch.zeros((B * g * g, Kpad), dtype=img.dtype)
    out[:, :K] = img.view(B, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, K)
    return out


def first_last_max(ids):
    """ids int64 [N, L] -> (column of the first maximum, of the last) per row."""
    pos = torch.arange(ids.shape[1])[None].expand_as(ids)
    top = ids == ids.max(dim=1, keepdim=True).values
    return torch.where(top, pos, ids.shape[1]).min(dim=1).values, torch.where(top, pos, -1).max(dim=1).values


def _attend(q, k, v, causal):
    """q [B, H, Lq, 64], k / v [B, H, L, 64] -> [B, Lq, H * 64] (multi_head_attention's arithmetic: scaled scores, additive mask, softmax)."""
    s = (q @ k.transpose(-1, -2)) * 0.125
    if causal:
        Lq, L = s.shape[-2:]
        s = s + torch.full((Lq, L), float("-inf"), dtype=s.dtype).triu_(1)
    o = s.softmax(dim=-1) @ v
    return o.transpose(1, 2).reshape(q.shape[0], q.shape[2], -1)


class Torch(Backend):
    """Every step in plain torch on flat CPU buffers of ONE dtype, nothing rounded in between.  weights / inputs: name -> tensor."""

    def __init__(self, weights, inputs, dt=torch.float64, n_cu=N_CU):
        super().__init__(n_cu)
        self.dt, self.buf = dt, {}
        for k, v in list(weights.items()) + list(inputs.items()):
            self.buf[k] = v.reshape(-1).to(dt if v.is_floating_point() else torch.int64)

    def alloc(self, name, elems, kind="f16"):
        if name not in self.buf or self.buf[name].numel() < elems:
            self.buf[name] = torch.zeros(elems, dtype=torch.int64 if kind == "i32" else self.dt)

    def m(self, r, rows, cols, ld=None):
        r = ref(r)
        return torch.as_strided(self.buf[r.name], (rows, cols), (cols if ld is None else ld, 1), r.off)

    def v(self, r, n):
        r = ref(r)
        return self.buf[r.name][r.off:r.off + n]

    def _ln(self, X, g, b):
        D = X.shape[-1]
        return F.layer_norm(X, (D,), self.v(g, D), self.v(b, D), 1e-5)

    # -- the hooks
    def gemm(self, f32, variant, A, W, C, M, N, K, epi, ldc, bias=None, res=None, pos=None, rows_in=0, rows_out=0, stats=None):
        acc = self.m(A, M, K) @ self.m(W, N, K).t()
        if epi in (EPI_BIAS, EPI_BIAS_QGELU, EPI_BIAS_RES):
            acc = acc + self.v(bias, N)
        if epi == EPI_BIAS_QGELU:
            acc = _gelu(acc)
        if epi == EPI_BIAS_RES:
            acc = acc + self.m(res, M, N, ldc)
        if epi == EPI_PATCH:
            m = torch.arange(M)
            b, p = m // rows_in, m % rows_in
            self.m(C, (M // rows_in) * rows_out, N, ldc)[b * rows_out + 1 + p] = acc + self.m(pos, rows_in + 1, N)[1 + p]
        else:
            self.m(C, M, N, ldc).copy_(acc)

    def gemm_patches(self, variant, image, R, W, pos, C, B, N):
        g2 = (R >> 4) ** 2
        col = _unfold(self.v(image, B * 3 * R * R).view(B, 3, R, R), 16, 768)
        acc = col @ self.m(W, N, 768).t()
        p = torch.arange(B * g2) % g2
        self.m(C, B, (g2 + 1) * N)[:, N:] = (acc + self.m(pos, g2 + 1, N)[1 + p]).view(B, g2 * N)

    def gemm_strided(self, variant, A, lda, W, ldw, bias, res, ldres, C, ldc, M, N, K, epi):
        assert epi == EPI_BIAS_RES
        acc = self.m(A, M, K, lda) @ self.m(W, N, K, ldw).t() + self.v(bias, N) + self.m(res, M, N, ldres)
        self.m(C, M, N, ldc).copy_(acc)

    def lnfold(self, variant, A1, W1, b1, res, M, D, K1, W2, gamma, beta, b2, N2, qgelu, x1, C2):
        if A1 is not None:
            self.m(x1, M, D).copy_(self.m(A1, M, K1) @ self.m(W1, D, K1).t() + self.v(b1, D) + self.m(res, M, D))
        acc = self._ln(self.m(x1, M, D), gamma, beta) @ self.m(W2, N2, D).t() + self.v(b2, N2)
        self.m(C2, M, N2).copy_(_gelu(acc) if qgelu else acc)

    def layernorm(self, f32, x, y, g, b, rows, D, in_stride):
        self.m(y, rows, D).copy_(self._ln(self.m(x, rows, D, in_stride).clone(), g, b))

    def attention(self, f32, variant, qkv, out, B, L, H, causal, engine=None):
        self.attention_q(variant, qkv, out, B, L, L, H, causal)

    def attention_q(self, variant, qkv, out, B, L, Lq, H, causal):
        q, k, v = self.m(qkv, B * L, 3 * H * 64).view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
        self.m(out, B * Lq, H * 64).copy_(_attend(q[:, :, :Lq], k, v, causal).reshape(B * Lq, H * 64))

    def attention_f32_varlen(self, qkv, out, offsets, nseq, n_ctx, max_len, H):
        D = H * 64
        for c in range(nseq):
            r0, r1 = (c * max_len, (c + 1) * max_len) if offsets is None else (offsets[c] + c * n_ctx, offsets[c + 1] + (c + 1) * n_ctx)
            self.attention(1, 0, Ref(ref(qkv).name, ref(qkv).off + r0 * 3 * D), Ref(ref(out).name, ref(out).off + r0 * D), 1, r1 - r0, H, 0)

    attention_f32_long = attention_f32_varlen

    def l2norm(self, x, rows, D, times):
        X = self.m(x, rows, D)
        for _ in range(times):
            X.copy_(X / X.norm(dim=-1, keepdim=True))

    def text_ensemble(self, feats, T, rows, E, out):
        f = self.m(feats, T * rows, E).view(T, rows, E)
        mean = (f / f.norm(dim=-1, keepdim=True)).mean(dim=0)
        self.m(out, rows, E).copy_(mean / mean.norm(dim=-1, keepdim=True))

    def text_embed_ids(self, ids, ids_stride, tok, pos, x, index, N, Lctx, Lseq, D):
        t = self.m(ids, N, Lctx, ids_stride)
        table = self.buf[ref(tok).name].view(-1, D)
        self.m(x, N * Lseq, D).copy_((table[t[:, :Lseq]] + self.m(pos, Lseq, D)[None]).reshape(N * Lseq, D))
        self.v(index, N).copy_(first_last_max(t)[0])

    def set_index(self, index, ids, N, Lctx):
        self.v(index, N).copy_(first_last_max(self.m(ids, N, Lctx))[1])

    def text_add_pos(self, prompts, Lctx, pos, x, N, Lseq, D):
        p = self.m(prompts, N, Lctx * D).view(N, Lctx, D)[:, :Lseq]
        self.m(x, N * Lseq, D).copy_((p + self.m(pos, Lseq, D)[None]).reshape(N * Lseq, D))

    def gather_rows(self, x, index, out, N, Lseq, D):
        i = self.v(index, N).clamp(0, Lseq - 1)
        self.m(out, N, D).copy_(self.m(x, N * Lseq, D).view(N, Lseq, D)[torch.arange(N), i])

    def im2col(self, image, f32, B, R, P, Kpad, out):
        self.m(out, B * (R // P) ** 2, Kpad).copy_(_unfold(self.v(image, B * 3 * R * R).view(B, 3, R, R), P, Kpad))

    def fill_cls(self, x, cls, B, L, W):
        self.m(x, B, W, L * W).copy_(self.v(cls, W)[None].expand(B, W))

    # -- the two copies
    def agg_input(self, feats, cls, x, first, shots, n_ctx, D):
        f, c = self.buf[ref(feats).name].view(-1, D), self.v(cls, n_ctx * D).view(n_ctx, D)
        self.m(x, sum(n_ctx + n for n in shots), D).copy_(torch.cat([t for src in first for t in (c, f[src])]))

    def agg_output(self, x, tokens, starts, n_ctx, D):
        for c, r0 in enumerate(starts):
            self.m(Ref(ref(tokens).name, ref(tokens).off + c * n_ctx * D), n_ctx, D).copy_(self.m(Ref(ref(x).name, ref(x).off + r0 * D), n_ctx, D))


class Hooks(Backend):
    """Every step as ONE call of the library's debug hook of that name on device buffers; a non-zero return code raises.  weights: name ->
    tensor as the library stores it (fp16 / fp32), inputs as the entry point takes them.  Every buffer has PAD elements of slack.
    fill (a name of poison.FILLS): every buffer instead comes from a poison.Arena under that fill -- the scratch of alloc, and guarded
    copies of the weights, the inputs and the offset tables --, with one 256-row tile of the widest weight row (4 * width: the widest
    row of any operand) in front of each operand and behind it, and the operand itself starting as the fill.  Weights handed over as a
    poison.Placed are guarded already (one copy shared by several replays) and used as they are."""
    PAD = 4096
    KINDS = {"f16": torch.float16, "f32": torch.float32, "i32": torch.int32}

    def __init__(self, lib, weights, inputs, n_cu, device="cuda", fill=None):
        super().__init__(n_cu)
        self.lib, self.device, self.keep, self.arena = lib, device, [], None
        if fill is None:
            self.buf = {k: v for k, v in weights.items()}
            self.buf.update({k: v.contiguous().to(device) for k, v in inputs.items()})
            return
        import poison
        if isinstance(weights, poison.Placed):                # guarded already, by a caller who shares them among replays
            assert weights.arena.fill == fill and str(weights.arena.device) == str(device)
            self.arena = poison.Arena(fill, device, weights.arena.guard)
            self.buf = dict(weights)
            weights = {}
        else:
            self.arena = poison.Arena(fill, device, poison.guard_elems(self.widest_row(weights)))
            self.buf = {}
        self.buf.update({k: self.arena.place(v) for k, v in list(weights.items()) + list(inputs.items())})

    @staticmethod
    def widest_row(weights):
        """The widest row of any operand: 4 * width, the K of c_proj (and the N of c_fc)."""
        return max([v.shape[-1] for v in weights.values() if v.dim() >= 1], default=16)

    def alloc(self, name, elems, kind="f16"):
        if self.arena is not None:
            if name not in self.buf or self.buf[name].numel() < elems:
                self.buf[name] = self.arena.take(elems, kind)
        elif name not in self.buf or self.buf[name].numel() < elems + self.PAD:
            self.buf[name] = torch.zeros(elems + self.PAD, dtype=self.KINDS[kind], device=self.device)

    def p(self, r):
        if r is None:
            return None
        r = ref(r)
        t = self.buf[r.name]
        assert 0 <= r.off < max(1, t.numel()), r
        return ctypes.c_void_p(t.data_ptr() + r.off * t.element_size())

    def t(self, r, n):
        r = ref(r)
        return self.buf[r.name].reshape(-1)[r.off:r.off + n]

    def call(self, fn, *args):
        rc = getattr(self.lib, "ovmr_debug_" + fn)(*args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RuntimeError(f"ovmr_debug_{fn} returned {rc}: {self.plan[-1]}")

    def gemm(self, f32, variant, A, W, C, M, N, K, epi, ldc, bias=None, res=None, pos=None, rows_in=0, rows_out=0, stats=None):
        assert stats is None or (epi == EPI_BIAS_RES and pos is None)          # the statistics epilogue: handed over as `pos`
        self.call("gemm", f32, variant, self.p(A), self.p(W), self.p(bias), self.p(res), self.p(pos if stats is None else stats), self.p(C),
                  M, N, K, ldc, epi, 1.0, rows_in, rows_out)

    def gemm_patches(self, variant, image, R, W, pos, C, B, N):
        self.call("gemm_patches", variant, self.p(image), R, self.p(W), self.p(pos), self.p(C), B, N)

    def gemm_strided(self, variant, A, lda, W, ldw, bias, res, ldres, C, ldc, M, N, K, epi):
        self.call("gemm_strided", variant, self.p(A), lda, self.p(W), ldw, self.p(bias), self.p(res), ldres, self.p(C), ldc, M, N, K, epi, 1.0,
                  None, None, 1)

    def lnfold(self, variant, A1, W1, b1, res, M, D, K1, W2, gamma, beta, b2, N2, qgelu, x1, C2):
        self.call("lnfold", variant, self.p(A1), self.p(W1), self.p(b1), self.p(res), M, D, K1, self.p(W2), self.p(gamma), self.p(beta),
                  self.p(b2), N2, qgelu, self.p(x1), self.p(C2))

    def layernorm(self, f32, x, y, g, b, rows, D, in_stride):
        self.call("layernorm", f32, self.p(x), self.p(y), self.p(g), self.p(b), rows, D, in_stride)

    def attention(self, f32, variant, qkv, out, B, L, H, causal, engine=None):
        self.call("attention", f32, variant, self.p(qkv), self.p(out), B, L, H, causal)

    def attention_q(self, variant, qkv, out, B, L, Lq, H, causal):
        self.call("attention_q", variant, self.p(qkv), self.p(out), B, L, Lq, H, causal)

    def _table(self, offsets):
        if offsets is None:
            return None
        table = torch.tensor(offsets, dtype=torch.int32)
        self.keep.append(table.to(self.device) if self.arena is None else self.arena.place(table))
        return ctypes.c_void_p(self.keep[-1].data_ptr())

    def attention_f32_varlen(self, qkv, out, offsets, nseq, n_ctx, max_len, H):
        self.call("attention_f32_varlen", self.p(qkv), self.p(out), self._table(offsets), nseq, n_ctx, max_len, H)

    def attention_f32_long(self, qkv, out, offsets, nseq, n_ctx, max_len, H):
        self.call("attention_f32_long", self.p(qkv), self.p(out), self._table(offsets), nseq, n_ctx, max_len, H)

    def l2norm(self, x, rows, D, times):
        self.call("l2norm", self.p(x), rows, D, times)

    def text_ensemble(self, feats, T, rows, E, out):
        self.call("text_ensemble", self.p(feats), T, rows, E, self.p(out))

    def text_embed_ids(self, ids, ids_stride, tok, pos, x, index, N, Lctx, Lseq, D):
        self.call("text_embed_ids", self.p(ids), ids_stride, self.p(tok), self.p(pos), self.p(x), self.p(index), N, Lctx, Lseq, D)

    def set_index(self, index, ids, N, Lctx):
        self.t(index, N).copy_(first_last_max(self.t(ids, N * Lctx).view(N, Lctx).cpu())[1].to(torch.int32))

    def text_add_pos(self, prompts, Lctx, pos, x, N, Lseq, D):
        self.call("text_add_pos", self.p(prompts), Lctx, self.p(pos), self.p(x), N, Lseq, D)

    def gather_rows(self, x, index, out, N, Lseq, D):
        self.call("gather_rows", self.p(x), self.p(index), self.p(out), N, Lseq, D)

    def im2col(self, image, f32, B, R, P, Kpad, out):
        self.call("im2col", self.p(image), f32, B, R, P, Kpad, self.p(out))

    def fill_cls(self, x, cls, B, L, W):
        self.call("fill_cls", self.p(x), self.p(cls), B, L, W)

    def agg_input(self, feats, cls, x, first, shots, n_ctx, D):
        f, c = self.buf[ref(feats).name].view(-1, D).float(), self.t(cls, n_ctx * D).view(n_ctx, D)
        self.t(x, sum(n_ctx + n for n in shots) * D).copy_(torch.cat([t for src in first for t in (c, f[src])]).reshape(-1))

    def agg_output(self, x, tokens, starts, n_ctx, D):
        for c, r0 in enumerate(starts):
            self.t(Ref(ref(tokens).name, ref(tokens).off + c * n_ctx * D), n_ctx * D).copy_(self.t(Ref(ref(x).name, ref(x).off + r0 * D), n_ctx * D))


# ---- the block both fp16 towers run ---------------------------------------------------------------------------------------------

MUTATIONS = {
    # image tower
    "img_pos_row": "positional row p + 1 taken as p",
    "res_from_y": "the residual of out_proj read from y (either fp16 tower)",
    "img_last_res_row1": "the last block's residual read from token row 1",
    "img_ln_post_pre": "ln_post with ln_pre's parameters",
    "img_proj_not_transposed": "proj not transposed (vision width == embed_dim)",
    "norm_once_more": "one normalisation more",
    "swap_blocks": "blocks 0 and 1 swapped (either fp16 tower)",
    "img_seq2_images": "the second launch sequence reading the first one's images",
    # text tower
    "txt_not_causal": "causal = 0",
    "txt_last_max": "the read-out row at the last maximum of the ids instead of the first",
    "txt_row0": "group 2's rows starting at group 1's row0",
    "txt_index_off0": "a later ids group's index read from offset 0 of the shared table instead of n0",
    "txt_proj_rows": "group 2's projection run on group 1's rows of the read-out buffer",
    # generator
    "gen_next_first": "class c reading class c + 1's first exemplar",
    "gen_tail_rows": "n_ctx rows taken from the end",
    "gen_ln_swapped": "ln_1 and ln_2 parameters swapped",
}
# Not a mutation: ln_final applied before the gather instead of after -- the same per row.


def blocks_f16(be, o, prefix, n, M, W, fold, attention, mut, cls=None):
    """run_block_f16, n times, on the buffers x, y, qkv, hid (and stats, rows).  fold: ln_1 / ln_2 folded into in_proj / c_fc -- the
    engine's pairs of launches (the GEMM with the statistics epilogue, then the folded GEMM that consumes them) are the two chains of
    ovmr_debug_lnfold: out_proj with ln_2 + c_fc, c_proj of block i with ln_1 + in_proj of block i + 1; A1 = None for the first block,
    whose statistics come from the row-statistics pass.  attention(i): the tower's launch(es).  cls = (nseq, L): the last block
    runs on the CLS query only and leaves its rows in `rows`."""
    order = list(range(n))
    if mut == "swap_blocks" and n >= 2:
        order[0], order[1], be.hit = 1, 0, True
    w = lambda i, k: f"{prefix}{order[i]}.{k}"
    gv = o["gemm"]
    qv = gv if o["gelu_exact"] else gv + 100                  # the one-rounding QuickGELU: variant + 100 through the hooks
    for i in range(n):
        last_cls = cls is not None and i == n - 1
        if not fold:
            be.step("layernorm", f32=0, x="x", y="y", g=w(i, "ln_1.weight"), b=w(i, "ln_1.bias"), rows=M, D=W, in_stride=W)
            be.step("gemm", f32=0, variant=gv, A="y", W=w(i, "attn.in_proj_weight"), bias=w(i, "attn.in_proj_bias"), C="qkv",
                    M=M, N=3 * W, K=W, epi=EPI_BIAS, ldc=3 * W)
        elif i == 0:
            be.step("lnfold", variant=gv, A1=None, W1=None, b1=None, res=None, M=M, D=W, K1=0, W2=w(0, "attn.in_proj_weight"),
                    gamma=w(0, "ln_1.weight"), beta=w(0, "ln_1.bias"), b2=w(0, "attn.in_proj_bias"), N2=3 * W, qgelu=0, x1="x", C2="qkv")
        attention(i, last_cls)
        if last_cls:
            nseq, L = cls
            res = "x"
            if mut == "img_last_res_row1":
                res, be.hit = Ref("x", W), True
            be.step("gemm_strided", variant=gv, A="y", lda=W, W=w(i, "attn.out_proj.weight"), ldw=W, bias=w(i, "attn.out_proj.bias"),
                    res=res, ldres=L * W, C="rows", ldc=W, M=nseq, N=W, K=W, epi=EPI_BIAS_RES)
            be.step("layernorm", f32=0, x="rows", y="y", g=w(i, "ln_2.weight"), b=w(i, "ln_2.bias"), rows=nseq, D=W, in_stride=W)
            be.step("gemm", f32=0, variant=qv, A="y", W=w(i, "mlp.c_fc.weight"), bias=w(i, "mlp.c_fc.bias"), C="hid",
                    M=nseq, N=4 * W, K=W, epi=EPI_BIAS_QGELU, ldc=4 * W)
            be.step("gemm", f32=0, variant=gv, A="hid", W=w(i, "mlp.c_proj.weight"), bias=w(i, "mlp.c_proj.bias"), res="rows", C="rows",
                    M=nseq, N=W, K=4 * W, epi=EPI_BIAS_RES, ldc=W)
            continue
        res = "x"
        if mut == "res_from_y":
            res, be.hit = "y", True
        if fold:
            be.step("lnfold", variant=qv, A1="y", W1=w(i, "attn.out_proj.weight"), b1=w(i, "attn.out_proj.bias"), res=res, M=M, D=W, K1=W,
                    W2=w(i, "mlp.c_fc.weight"), gamma=w(i, "ln_2.weight"), beta=w(i, "ln_2.bias"), b2=w(i, "mlp.c_fc.bias"), N2=4 * W,
                    qgelu=1, x1="x", C2="hid")
            if i + 1 < n:
                be.step("lnfold", variant=gv, A1="hid", W1=w(i, "mlp.c_proj.weight"), b1=w(i, "mlp.c_proj.bias"), res="x", M=M, D=W,
                        K1=4 * W, W2=w(i + 1, "attn.in_proj_weight"), gamma=w(i + 1, "ln_1.weight"), beta=w(i + 1, "ln_1.bias"),
                        b2=w(i + 1, "attn.in_proj_bias"), N2=3 * W, qgelu=0, x1="x", C2="qkv")
            else:                                             # the statistics of the tower's last x: written, read by nothing
                be.step("gemm", f32=0, variant=gv, A="hid", W=w(i, "mlp.c_proj.weight"), bias=w(i, "mlp.c_proj.bias"), res="x", C="x",
                        M=M, N=W, K=4 * W, epi=EPI_BIAS_RES, ldc=W, stats="stats")
        else:
            be.step("gemm", f32=0, variant=gv, A="y", W=w(i, "attn.out_proj.weight"), bias=w(i, "attn.out_proj.bias"), res=res, C="x",
                    M=M, N=W, K=W, epi=EPI_BIAS_RES, ldc=W)
            be.step("layernorm", f32=0, x="x", y="y", g=w(i, "ln_2.weight"), b=w(i, "ln_2.bias"), rows=M, D=W, in_stride=W)
            be.step("gemm", f32=0, variant=qv, A="y", W=w(i, "mlp.c_fc.weight"), bias=w(i, "mlp.c_fc.bias"), C="hid",
                    M=M, N=4 * W, K=W, epi=EPI_BIAS_QGELU, ldc=4 * W)
            be.step("gemm", f32=0, variant=gv, A="hid", W=w(i, "mlp.c_proj.weight"), bias=w(i, "mlp.c_proj.bias"), res="x", C="x",
                    M=M, N=W, K=4 * W, epi=EPI_BIAS_RES, ldc=W)


def _tower_buffers(be, M, N, W, col=0):
    be.alloc("col", col)
    be.alloc("x", M * W)
    be.alloc("y", M * W)
    be.alloc("qkv", M * 3 * W)
    be.alloc("hid", M * 4 * W)
    be.alloc("rows", N * W)
    be.alloc("stats", M * ((W + 255) // 256) * 2, "f32")


# ---- image tower (clip/model.py:411-428; ovmr_encode_image) -----------------------------------------------------------------------

def image_tower(be, case, mut=None):
    """-> "out" [B, embed_dim].  args: B, f32 (fp32 images), normalize."""
    s, o = SPECS[case.spec], options(case)
    W, R, P, E = s.vision_width, s.image_resolution, s.vision_patch_size, s.embed_dim
    G2, L, H, Kpad, n = s.grid ** 2, s.vision_tokens, W // 64, (3 * P * P + 63) // 64 * 64, s.vision_layers
    B, f32, normalize = case.args["B"], bool(case.args.get("f32")), int(case.args.get("normalize", 1))
    seqs = encode_plan(case, be.n_cu)
    _tower_buffers(be, max(seqs) * L, max(seqs), W, max(seqs) * G2 * Kpad)
    be.alloc("out", B * E)
    b0 = 0
    for si, Bc in enumerate(seqs):
        if Bc >= 256 and o["last_q_cls"]:
            raise ValueError(f"{case.name}: a launch sequence of {Bc} images needs last_q_cls = 0 (module docstring)")
        M, src = Bc * L, b0
        if mut == "img_seq2_images" and si == 1:
            src, be.hit = 0, True
        image, pos = Ref("image", src * 3 * R * R), "pos16_vis"
        if mut == "img_pos_row":
            pos, be.hit = "pos16_vis_shift", True
        # the engine's fused_patches rule (the image pointer of a torch tensor is 16-byte aligned, and so is every image behind it)
        if o["fuse_im2col"] and not f32 and P == 16 and Kpad == 768 and R % 16 == 0 and Bc * G2 >= 256 and W >= 128 and o["gemm"] >= 1:
            be.step("gemm_patches", variant=o["gemm"], image=image, R=R, W="conv_w", pos=pos, C="x", B=Bc, N=W)
        else:
            be.step("im2col", image=image, f32=int(f32), B=Bc, R=R, P=P, Kpad=Kpad, out="col")
            be.step("gemm", f32=0, variant=o["gemm"], A="col", W="conv_w", pos=pos, C="x", M=Bc * G2, N=W, K=Kpad, epi=EPI_PATCH, ldc=W,
                    rows_in=G2, rows_out=L)
        be.step("fill_cls", x="x", cls="cls_pos16", B=Bc, L=L, W=W)
        be.step("layernorm", f32=0, x="x", y="x", g="visual.ln_pre.weight", b="visual.ln_pre.bias", rows=M, D=W, in_stride=W)

        def attention(i, last_cls):
            if last_cls:
                be.step("attention_q", variant=o["attn"], qkv="qkv", out="y", B=Bc, L=L, Lq=1, H=H, causal=0)
            else:
                be.step("attention", f32=0, variant=o["attn"], qkv="qkv", out="y", B=Bc, L=L, H=H, causal=0)
        blocks_f16(be, o, "visual.transformer.resblocks.", n, M, W, can_fold(o, M, W), attention, mut, cls=(Bc, L))
        post = "visual.ln_post"
        if mut == "img_ln_post_pre":
            post, be.hit = "visual.ln_pre", True
        be.step("layernorm", f32=0, x="rows", y="rows", g=post + ".weight", b=post + ".bias", rows=Bc, D=W, in_stride=W)
        proj = "proj_t"
        if mut == "img_proj_not_transposed" and W == E:
            proj, be.hit = "proj_nt", True
        out = Ref("out", b0 * E)
        be.step("gemm", f32=0, variant=o["gemm"], A="rows", W=proj, C=out, M=Bc, N=E, K=W, epi=EPI_NONE, ldc=E)
        _normalize(be, out, Bc, E, 1 if normalize else 0, mut)
        b0 += Bc
    return "out"


def _normalize(be, x, rows, D, times, mut, normalized_later=False):
    if mut == "norm_once_more":
        # on rows that are normalised already, or will be (the ensemble's first step), one more is the identity but for its roundings
        be.rounding_only = (times > 0 or normalized_later) and (be.rounding_only or not be.hit)
        be.hit = True
        times += 1
    if times:
        be.step("l2norm", x=x, rows=rows, D=D, times=times)


# ---- text tower (clip/model.py:824-831; run_text_groups, run_text_group_chunked, the three entry points) ----------------------------

def text_groups_pass(be, case, groups, mut):
    """run_text_groups: groups = dicts with kind "ids" | "emb", their operands as Refs (ids / prompts, index), N, Ls, normalize, out."""
    s, o = SPECS[case.spec], options(case)
    W, Lc, E, n, H = s.transformer_width, s.context_length, s.embed_dim, s.transformer_layers, s.transformer_width // 64
    row0, M = [], 0
    for g in groups:
        row0.append(M)
        M += g["N"] * g["Ls"]
    N = sum(g["N"] for g in groups)
    assert text_rows_fit(M, N, W), case.name
    _tower_buffers(be, M, N, W)
    be.alloc("index", N, "i32")
    n0 = 0
    for i, g in enumerate(groups):
        r0 = row0[i]
        if mut == "txt_row0" and i == 1:
            r0, be.hit = row0[0], True
        if g["kind"] == "ids":
            be.step("text_embed_ids", ids=g["ids"], ids_stride=Lc, tok="token_embedding.weight", pos="pos16_txt", x=Ref("x", r0 * W),
                    index=Ref("index", n0), N=g["N"], Lctx=Lc, Lseq=g["Ls"], D=W)
            if mut == "txt_last_max":
                be.hit = True
                be.step("set_index", index=Ref("index", n0), ids=g["ids"], N=g["N"], Lctx=Lc)
        else:
            be.step("text_add_pos", prompts=g["prompts"], Lctx=Lc, pos="pos16_txt", x=Ref("x", r0 * W), N=g["N"], Lseq=g["Ls"], D=W)
        n0 += g["N"]
    causal = 1
    if mut == "txt_not_causal":
        causal, be.hit = 0, True
    one_launch = o["attn"] >= 1 and len(groups) <= 4 and all(g["Ls"] <= 32 for g in groups)

    def attention(i, last_cls):
        for r0, g in zip(row0, groups):                       # one launch per group, whichever launch the engine used
            be.step("attention", f32=0, variant=o["attn"], qkv=Ref("qkv", r0 * 3 * W), out=Ref("y", r0 * W), B=g["N"], L=g["Ls"], H=H,
                    causal=causal, engine="one launch for the groups" if one_launch else "a launch per group")
    blocks_f16(be, o, "transformer.resblocks.", n, M, W, n > 0 and can_fold(o, M, W), attention, mut)
    n0 = 0
    for i, g in enumerate(groups):
        index = Ref("index", n0) if g["kind"] == "ids" else g["index"]
        if mut == "txt_index_off0" and g["kind"] == "ids" and n0 > 0:
            index, be.hit = Ref("index", 0), True
        be.step("gather_rows", x=Ref("x", row0[i] * W), index=index, out=Ref("rows", n0 * W), N=g["N"], Lseq=g["Ls"], D=W)
        n0 += g["N"]
    be.step("layernorm", f32=0, x="rows", y="rows", g="ln_final.weight", b="ln_final.bias", rows=N, D=W, in_stride=W)
    n0 = 0
    for i, g in enumerate(groups):
        rows = Ref("rows", n0 * W)
        if mut == "txt_proj_rows" and i == 1:
            rows, be.hit = Ref("rows", 0), True
        be.step("gemm", f32=0, variant=o["gemm"], A=rows, W="textproj_t", C=g["out"], M=g["N"], N=E, K=W, epi=EPI_NONE, ldc=E)
        _normalize(be, g["out"], g["N"], E, g["normalize"], mut, g.get("normalized_later", False))
        n0 += g["N"]


def text_tower(be, case, mut=None):
    """-> the output buffers' names.  entry encode_text_groups: args groups = [(kind, N, Ls, normalize)], ONE pass; encode_text_ids /
    encode_text_embedded: ONE such group in chunks of max_prompts sequences; encode_text_ensemble: args T, C, seq_lens -- T groups of C
    prompts (ids template-major), un-normalised into `raw`, then ovmr_debug_text_ensemble."""
    s = SPECS[case.spec]
    W, Lc, E = s.transformer_width, s.context_length, s.embed_dim
    if case.entry == "encode_text_ensemble":
        T, C, lens = case.args["T"], case.args["C"], case.args["seq_lens"]
        be.alloc("raw", T * C * E)
        be.alloc("out", C * E)
        groups = [{"kind": "ids", "ids": Ref("ids", t * C * Lc), "N": C, "Ls": lens[t], "normalize": 0, "out": Ref("raw", t * C * E),
                   "normalized_later": True} for t in range(T)]
        text_groups_pass(be, case, groups, mut)
        be.step("text_ensemble", feats="raw", T=T, rows=C, E=E, out="out")
        return ["out"]
    outs = []
    specs = case.args["groups"]
    for i, (kind, N, Ls, normalize) in enumerate(specs):
        be.alloc(f"out{i}", N * E)
        outs.append(f"out{i}")
    if case.entry == "encode_text_groups":
        groups = [{"kind": kind, "ids": Ref(f"ids{i}"), "prompts": Ref(f"prompts{i}"), "index": Ref(f"index{i}"), "N": N, "Ls": Ls,
                   "normalize": normalize, "out": Ref(f"out{i}")} for i, (kind, N, Ls, normalize) in enumerate(specs)]
        text_groups_pass(be, case, groups, mut)
        return outs
    (kind, N, Ls, normalize), cap = specs[0], case.reserve[1]
    assert len(specs) == 1 and case.entry == ("encode_text_ids" if kind == "ids" else "encode_text_embedded")
    for n0 in range(0, N, cap):                               # run_text_group_chunked
        g = {"kind": kind, "ids": Ref("ids0", n0 * Lc), "prompts": Ref("prompts0", n0 * Lc * W), "index": Ref("index0", n0),
             "N": min(cap, N - n0), "Ls": Ls, "normalize": normalize, "out": Ref("out0", n0 * E)}
        text_groups_pass(be, case, [g], mut)
    return outs


# ---- visual-token generator (trainers/mm_classifier_one_prompt.py:167-169; generate_tokens, run_block_f32) -----------------------------

def generator(be, case, mut=None):
    """-> "out" [Cb, n_ctx, D] fp32.  args: shots (one count per class) and uniform (ovmr_generate_tokens: no table) or not."""
    s, o = SPECS[case.spec], options(case)
    D, H, n_ctx = s.embed_dim, s.embed_dim // 64, N_CTX
    shots, uniform = list(case.args["shots"]), bool(case.args["uniform"])
    Cb, cap = len(shots), case.reserve[2] * (n_ctx + 32)
    assert not uniform or len(set(shots)) == 1
    lens = [n_ctx + n for n in shots]
    assert max(lens) <= o["agg_max_len"], case.name
    first = [sum(shots[:c]) for c in range(Cb + 1)]           # the exclusive prefix sum of the shots: the device table
    be.alloc("out", Cb * n_ctx * D, "f32")
    c0 = 0
    while c0 < Cb:                                            # chunks: runs of whole classes whose rows fit the capacity, at least one
        c1, rows = c0, 0
        while c1 < Cb and (c1 == c0 or rows + lens[c1] <= cap):
            rows += lens[c1]
            c1 += 1
        Cc, max_len = c1 - c0, max(lens[c0:c1])
        for name, k in (("ax", 1), ("ay", 1), ("aqkv", 3), ("ahid", 4)):
            be.alloc(name, rows * k * D, "f32")
        src = [list(range(first[c], first[c + 1])) for c in range(c0, c1)]
        if mut == "gen_next_first":
            for c in range(c0, c1):
                if c + 1 < Cb:
                    src[c - c0][0], be.hit = first[c + 1], True
        be.step("agg_input", feats="feats", cls="prompt_learner.cls_token", x="ax", first=src, shots=shots[c0:c1], n_ctx=n_ctx, D=D)
        offsets = None if uniform else [first[c] - first[c0] for c in range(c0, c1 + 1)]
        ln = ("ln_1", "ln_2")
        if mut == "gen_ln_swapped":
            ln, be.hit = ("ln_2", "ln_1"), True
        for i in range(s.agg_layers):                         # run_block_f32: seven launches
            w = lambda k: f"prompt_learner.aggregator.resblocks.{i}.{k}"
            be.step("layernorm", f32=1, x="ax", y="ay", g=w(ln[0] + ".weight"), b=w(ln[0] + ".bias"), rows=rows, D=D, in_stride=D)
            be.step("gemm", f32=1, variant=0, A="ay", W=w("attn.in_proj_weight"), bias=w("attn.in_proj_bias"), C="aqkv", M=rows, N=3 * D, K=D,
                    epi=EPI_BIAS, ldc=3 * D)
            if max_len > 128:
                be.step("attention_f32_long", qkv="aqkv", out="ay", offsets=offsets, nseq=Cc, n_ctx=n_ctx, max_len=max_len, H=H)
            elif uniform:
                be.step("attention", f32=1, variant=0, qkv="aqkv", out="ay", B=Cc, L=max_len, H=H, causal=0)
            else:
                be.step("attention_f32_varlen", qkv="aqkv", out="ay", offsets=offsets, nseq=Cc, n_ctx=n_ctx, max_len=max_len, H=H)
            be.step("gemm", f32=1, variant=0, A="ay", W=w("attn.out_proj.weight"), bias=w("attn.out_proj.bias"), res="ax", C="ax", M=rows,
                    N=D, K=D, epi=EPI_BIAS_RES, ldc=D)
            be.step("layernorm", f32=1, x="ax", y="ay", g=w(ln[1] + ".weight"), b=w(ln[1] + ".bias"), rows=rows, D=D, in_stride=D)
            be.step("gemm", f32=1, variant=0, A="ay", W=w("mlp.c_fc.weight"), bias=w("mlp.c_fc.bias"), C="ahid", M=rows, N=4 * D, K=D,
                    epi=EPI_BIAS_QGELU, ldc=4 * D)
            be.step("gemm", f32=1, variant=0, A="ahid", W=w("mlp.c_proj.weight"), bias=w("mlp.c_proj.bias"), res="ax", C="ax", M=rows,
                    N=D, K=4 * D, epi=EPI_BIAS_RES, ldc=D)
        starts, r = [], 0
        for c in range(c0, c1):
            starts.append(r)
            r += lens[c]
        if mut == "gen_tail_rows":
            starts, be.hit = [r0 + lens[c0 + j] - n_ctx for j, r0 in enumerate(starts)], True
        be.step("agg_output", x="ax", tokens=Ref("out", c0 * n_ctx * D), starts=starts, n_ctx=n_ctx, D=D)
        c0 = c1
    return "out"


PATHS = {"image": image_tower, "text": text_tower, "gen": generator}


def run(be, case, mut=None):
    """The case's path on `be` -> the output buffers' names (a list)."""
    out = PATHS[case.path](be, case, mut)
    return out if isinstance(out, list) else [out]


def plan(case, n_cu=N_CU):
    """The launches of the case, in order: pure, no GPU."""
    be = Planner(n_cu)
    run(be, case)
    return be.plan


def mutations_of(case, n_cu=N_CU, identities=False):
    """The mutations whose step the case runs.  "One normalisation more" on rows that are normalised already (or will be) is the
    identity in exact arithmetic, and in fp16 as good as always too (the norm of a normalised row rounds to 1): no defect there, and
    left out unless `identities` asks for exactly those."""
    out = []
    for m in MUTATIONS:
        be = Planner(n_cu)
        run(be, case, m)
        if be.hit and be.rounding_only == identities:
            out.append(m)
    return out


def show_plan(p):
    return "\n".join("  " + ", ".join(f"{k}={v}" for k, v in r.items() if v is not None) for r in p)


# ---- weights and inputs -----------------------------------------------------------------------------------------------------------

SEED = 5
_HALF = ("attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "mlp.c_fc.weight", "mlp.c_fc.bias",
         "mlp.c_proj.weight", "mlp.c_proj.bias")
_HALF_SINGLE = ("visual.proj", "text_projection", "visual.conv1.weight")


@functools.lru_cache(maxsize=None)
def state_dicts(spec):
    """(CLIP state dict, prompt learner's) of SPECS[spec] as fp32 torch tensors: jitter = True, so no gamma is 1 and no bias is 0."""
    s = SPECS[spec]
    sd = {k: torch.from_numpy(v) for k, v in synth.clip_state_dict(s, SEED, jitter=True).items()}
    pl = {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(s, N_CTX, SEED, jitter=True).items()}
    return sd, pl


def weights(spec, rnd, keep):
    """name -> tensor: the state dict as ovmr_set_weight stores it (rnd: the tensors convert_weights halves, clip/model.py:852-873;
    keep: LayerNorm parameters, embeddings, the whole aggregator) and the layouts ovmr_finalize derives from it:
    conv_w [W, Kpad] zero-padded, pos16_vis / pos16_txt = h(pos), cls_pos16 = h(h(class_embedding) + h(pos[0])), proj_t / textproj_t
    transposed.  For the mutations: pos16_vis_shift (row p + 1 holds row p) and proj_nt (as stored)."""
    s = SPECS[spec]
    sd, pl = state_dicts(spec)
    w = {k: (rnd(v) if k.endswith(_HALF) or k in _HALF_SINGLE else keep(v)) for k, v in sd.items() if k != "logit_scale"}
    w.update({"prompt_learner." + k: keep(v) for k, v in pl.items()})
    W, K = s.vision_width, 3 * s.vision_patch_size ** 2
    conv = w["visual.conv1.weight"].reshape(W, K)
    w["conv_w"] = torch.zeros((W, (K + 63) // 64 * 64), dtype=conv.dtype)
    w["conv_w"][:, :K] = conv
    pos = rnd(w["visual.positional_embedding"])
    w["pos16_vis"], w["pos16_vis_shift"] = pos, torch.cat([pos[:1], pos[:-1]])
    w["cls_pos16"] = rnd(w["visual.class_embedding"]) + pos[0]
    w["proj_t"], w["proj_nt"] = w["visual.proj"].t().contiguous(), w["visual.proj"].contiguous()
    w["pos16_txt"] = rnd(w["positional_embedding"])
    w["textproj_t"] = w["text_projection"].t().contiguous()
    return w


def _ids(gen, N, Ls, Lc):
    """int64 [N, Lc]: SOT, tokens, EOT at a column of [2, Ls) -- row 0 at Ls - 1, the rest spread --, zeros behind; every odd row
    (Ls >= 5) has a SECOND EOT two columns on, still inside Ls (the read-out row is the first maximum)."""
    ids = torch.zeros((N, Lc), dtype=torch.int64)
    for r in range(N):
        eot = Ls - 1 if r == 0 or Ls < 5 else 2 + (7 * r + 3) % (Ls - 4 if r % 2 else Ls - 2)
        ids[r, 0] = SOT
        ids[r, 1:eot] = torch.randint(1, SOT, (eot - 1,), generator=gen)
        ids[r, eot] = EOT
        if r % 2 == 1 and eot + 2 < Ls:
            ids[r, eot + 1] = 7
            ids[r, eot + 2] = EOT
    return ids


def input_key(case):
    return case.path, case.spec, case.entry, sorted(case.args.items())


@functools.lru_cache(maxsize=None)
def _inputs(name):
    case = BY_NAME[name]
    s, a = SPECS[case.spec], case.args
    gen = torch.Generator().manual_seed(zlib.crc32(repr(input_key(case)).encode()))      # the options and the reserve do not reach the inputs
    Lc, W = s.context_length, s.transformer_width
    if case.path == "image":
        R = s.image_resolution
        img = torch.randn((a["B"], 3, R, R), generator=gen)
        return {"image": img if a.get("f32") else img.half()}
    if case.path == "gen":
        f = torch.randn((sum(a["shots"]), s.embed_dim), generator=gen)
        return {"feats": (f / f.norm(dim=-1, keepdim=True)).half()}
    if case.entry == "encode_text_ensemble":
        return {"ids": torch.stack([_ids(gen, a["C"], a["seq_lens"][t], Lc) for t in range(a["T"])])}
    out = {}
    for i, (kind, N, Ls, _) in enumerate(a["groups"]):
        if kind == "ids":
            out[f"ids{i}"] = _ids(gen, N, Ls, Lc)
        else:
            out[f"prompts{i}"] = (0.02 * torch.randn((N, Lc, W), generator=gen)).half()
            out[f"index{i}"] = torch.tensor([Ls - 1 if r == 0 else 1 + (5 * r + 2) % (Ls - 1) for r in range(N)], dtype=torch.int32)
    return out


def inputs(case):
    """name -> CPU tensor, as the engine's entry point takes them: fp16 (fp32 images where the case says so), int64 ids, int32 index."""
    return _inputs(case.name)


# ---- the cases --------------------------------------------------------------------------------------------------------------------

def _img(name, spec, B, reserve=None, opts=None, **args):
    args["B"] = B
    return Case(name, "image", spec, opts or {}, (reserve or B, 8, 8), "encode_image", args)


def _txt(name, spec, entry, args, max_prompts=64, opts=None):
    return Case(name, "text", spec, opts or {}, (4, max_prompts, 8), entry, args)


def _gen(name, spec, shots, uniform=False, max_classes=16, opts=None):
    return Case(name, "gen", spec, opts or {}, (4, 8, max_classes), "generate_tokens" if uniform else "generate_tokens_ragged",
                {"shots": tuple(shots), "uniform": uniform})


def _cases():
    c = []
    # image tower.  tiny: W = 128 never folds; 64 images make the 256 patch rows the gathering GEMM needs
    for spec in ("tiny", "tiny1"):
        c += [_img(f"img_{spec}_b1", spec, 1), _img(f"img_{spec}_b63", spec, 63), _img(f"img_{spec}_b64", spec, 64),
              _img(f"img_{spec}_b64_f32", spec, 64, f32=True)]
    c += [_img("img_tiny_b64_raw", "tiny", 64, normalize=0), _img("img_tiny_b3_f32_raw", "tiny", 3, f32=True, normalize=0)]
    # small: 16 images = 272 token rows (latency-bound under gemm 8: unfolded; folded under 0 and 6); 300 images = 5100 rows: folded,
    # and at least 256 images in the last block; a reserve of 16 given 40: three launch sequences
    for spec in ("small", "small1", "small2"):
        c += [_img(f"img_{spec}_b16", spec, 16), _img(f"img_{spec}_b300", spec, 300, opts={"last_q_cls": 0}),
              _img(f"img_{spec}_b40_r16", spec, 40, reserve=16)]
    c += [_img("img_small_b40_r16_raw", "small", 40, reserve=16, normalize=0)]
    # ViT-B/16 geometry, L = 197: 3 images = 591 rows unfolded, 8 = 1576 rows folded; attention 3 (the single-pass kernel) and 1
    for spec in ("b16x1", "b16x2"):
        for B in (3, 8):
            c += [_img(f"img_{spec}_b{B}_attn{a}", spec, B, opts={"attn": a}) for a in (3, 1)]
    # a reserve of two rounds of tiles on 256 CUs (516 row tiles: the fold slack is 6600 images) with the chunk pinned to 100: 6801
    # images run as 100, 100 and 100 + 6501, the remainder folded into the last chunk
    c += [_img("img_tiny_fold_remainder", "tiny", 6801, reserve=26400, opts={"enc_chunk": 100, "last_q_cls": 0})]
    # options crossed on the cheap geometries
    for gemm in (0, 6, 8):
        for attn in (0, 1, 3):
            if (gemm, attn) != (8, 3):
                c += [_img(f"img_tiny_b64_g{gemm}a{attn}", "tiny", 64, opts={"gemm": gemm, "attn": attn}),
                      _img(f"img_small_b16_g{gemm}a{attn}", "small", 16, opts={"gemm": gemm, "attn": attn})]
    for key in ("gelu_exact", "ln_fold", "fuse_im2col"):
        v = 1 - OPTION_DEFAULTS[key]
        c += [_img(f"img_tiny_b64_{key}{v}", "tiny", 64, opts={key: v}),
              _img(f"img_small_b300_{key}{v}", "small", 300, opts={key: v, "last_q_cls": 0}),
              _img(f"img_small_b16_g6_{key}{v}", "small", 16, opts={key: v, "gemm": 6})]

    # text tower
    mixed = [("emb", 3, 9, 2), ("ids", 4, 12, 1), ("ids", 2, 7, 0)]
    five = [("ids", 2, 6, 1), ("emb", 3, 9, 2), ("ids", 1, 5, 0), ("emb", 2, 11, 1), ("ids", 3, 8, 1)]
    longer = [("ids", 3, 8, 0), ("emb", 2, 40, 1), ("ids", 2, 10, 1)]
    for spec in ("small", "small1", "small2"):
        c += [_txt(f"txt_{spec}_ids", spec, "encode_text_ids", {"groups": [("ids", 5, 77, 0)]}),
              _txt(f"txt_{spec}_emb", spec, "encode_text_embedded", {"groups": [("emb", 4, 20, 1)]}),
              _txt(f"txt_{spec}_mixed3", spec, "encode_text_groups", {"groups": mixed}),
              _txt(f"txt_{spec}_five", spec, "encode_text_groups", {"groups": five}),
              _txt(f"txt_{spec}_longer", spec, "encode_text_groups", {"groups": longer})]
    c += [_txt("txt_small_ids_chunks", "small", "encode_text_ids", {"groups": [("ids", 11, 16, 1)]}, max_prompts=4),
          _txt("txt_small_emb_chunks", "small", "encode_text_embedded", {"groups": [("emb", 7, 13, 2)]}, max_prompts=3),
          _txt("txt_small_ensemble", "small", "encode_text_ensemble", {"T": 3, "C": 5, "seq_lens": (9, 12, 7)}),
          _txt("txt_small_ensemble7", "small", "encode_text_ensemble", {"T": 7, "C": 3, "seq_lens": (9, 12, 7, 8, 40, 6, 10)})]
    # head768: 18 prompts of 77 tokens = 1386 rows at width 768: folded; 6 groups of short prompts past the same bound
    for spec in ("head768", "head768x1"):
        c += [_txt(f"txt_{spec}_ids_fold", spec, "encode_text_ids", {"groups": [("ids", 18, 77, 1)]}),
              _txt(f"txt_{spec}_mixed_fold", spec, "encode_text_groups", {"groups": [("ids", 60, 12, 1), ("emb", 50, 14, 2), ("ids", 3, 9, 0)]}),
              _txt(f"txt_{spec}_mixed", spec, "encode_text_groups", {"groups": mixed})]
    for gemm in (0, 6, 8):
        for attn in (0, 1, 3):
            if (gemm, attn) != (8, 3):
                c += [_txt(f"txt_small_mixed3_g{gemm}a{attn}", "small", "encode_text_groups", {"groups": mixed}, opts={"gemm": gemm, "attn": attn})]
    c += [_txt("txt_small_mixed3_gelu_exact1", "small", "encode_text_groups", {"groups": mixed}, opts={"gelu_exact": 1})]
    # 300 token rows at width 256: folded under gemm 6
    fold6 = [("ids", 20, 10, 1), ("emb", 10, 10, 0)]
    c += [_txt("txt_small_fold_g6", "small", "encode_text_groups", {"groups": fold6}, opts={"gemm": 6})]
    for key in ("gelu_exact", "ln_fold"):
        v = 1 - OPTION_DEFAULTS[key]
        c += [_txt(f"txt_small_fold_g6_{key}{v}", "small", "encode_text_groups", {"groups": fold6}, opts={"gemm": 6, key: v}),
              _txt(f"txt_head768_ids_fold_{key}{v}", "head768", "encode_text_ids", {"groups": [("ids", 18, 77, 1)]}, opts={key: v})]

    # generator: uniform (Cb, S) = (3, 4); ragged shots; one class alone; a capacity of 34 rows: three chunks; a class of 130 rows
    for spec in ("tiny", "small"):
        c += [_gen(f"gen_{spec}_uniform", spec, (4, 4, 4), uniform=True),
              _gen(f"gen_{spec}_ragged", spec, (1, 16, 33, 126)),
              _gen(f"gen_{spec}_one_class", spec, (5,)),
              _gen(f"gen_{spec}_chunks", spec, (1, 16, 33, 126), max_classes=1),
              _gen(f"gen_{spec}_uniform_chunks", spec, (4,) * 7, uniform=True, max_classes=1),
              _gen(f"gen_{spec}_long", spec, (3, 128, 20), opts={"agg_max_len": 256})]
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
