"""The poison method proves itself on the CPU (poison.py): the table of the four fills, the guarded allocator, and three small torch
emulations of a tiled kernel with one planted defect each, run over arenas under every fill.  The detection matrix asserted at the end
is the argument for running four fills and not one:

    defect                                        nan16      ones       big
    tail masked by p * 0 instead of a select      differs    differs    == zero   (65504 * 0 = 0, NaN * 0 = NaN)
    spare tile row votes on moving the reference  == zero    == zero    differs   (NaN > x is false: a NaN row never votes)
    accumulator not initialised                   differs    differs    differs

and every clean emulation is bit-equal under all four.  An emulation sees memory as a kernel does: a flat buffer it may index past the
operand's end (torch.as_strided over the arena's allocation), so an over-read lands in the guard.

The new hook ovmr_debug_fill_workspace is declared, exported and refuses a NULL handle: no GPU needed.
"""
import ctypes
import math
import os
import re

import pytest
import torch

import engine_replay as ER
import poison as P
from conftest import REPO

NONZERO = ("nan16", "ones", "big")


# ---- the fills and the allocator --------------------------------------------------------------------------------------------------

def test_fills_table():
    assert list(P.FILLS) == ["zero", "nan16", "ones", "big"]
    assert P.FILLS == {"zero": 0x00000000, "nan16": 0x7E007E00, "ones": 0xFFFFFFFF, "big": 0x7BFF7BFF}
    z, n, o, b = (P.as_read(P.FILLS[k]) for k in P.FILLS)
    assert z == {"f16": (0.0, 0.0), "f32": 0.0, "i32": 0} and math.copysign(1.0, z["f32"]) == 1.0
    # nan16: quiet NaN pairs (exponent all ones, the top mantissa bit set), a finite fp32 of about 2^125, a large positive integer
    assert all(math.isnan(h) for h in n["f16"]) and 0x7E00 & 0x7C00 == 0x7C00 and 0x7E00 & 0x0200
    assert math.isfinite(n["f32"]) and 2.0 ** 125 <= n["f32"] < 2.0 ** 125 * 1.01 and n["i32"] == 0x7E007E00 > 1 << 30
    assert all(math.isnan(h) for h in o["f16"]) and math.isnan(o["f32"]) and o["i32"] == -1
    assert b["f16"] == (65504.0, 65504.0) and math.isfinite(b["f32"]) and 2.0 ** 120 <= b["f32"] < 2.0 ** 121 and b["i32"] == 0x7BFF7BFF > 1 << 30
    assert [P.int_fill(k) for k in P.FILLS] == [0, 1, 1, 1]


@pytest.mark.parametrize("fill", list(P.FILLS))
def test_arena_alignment_and_guards(fill):
    guard = P.guard_elems(24)
    assert guard == 256 * 24 > ER.Hooks.PAD
    a = P.Arena(fill, "cpu", guard)
    for kind, elems in (("f16", 1001), ("f32", 77), ("i32", 13), ("i64", 5), ("f16", 0)):
        v = a.take(elems, kind)
        assert v.dtype == P.KINDS[kind] and v.numel() == elems and v.is_contiguous()
        assert elems == 0 or v.data_ptr() % 256 == 0
        front, behind = a.guards(len(a.keep) - 1)
        assert front.numel() >= guard and behind.numel() >= guard
        if elems:
            es = v.element_size()
            assert front.data_ptr() + front.numel() * es == v.data_ptr() and v.data_ptr() + elems * es == behind.data_ptr()
        want = P.fill_(torch.empty(1, dtype=v.dtype), fill)
        for part in (front, v, behind):                        # the guards AND the operand start as the fill
            assert P.same_bits(part, want.expand(part.numel()).contiguous()) is None
        if kind in ("i32", "i64"):
            assert int(want) == (0 if fill == "zero" else 1)
        elif kind == "f16":
            assert int(want.view(torch.int16)) & 0xFFFF == P.FILLS[fill] & 0xFFFF == P.FILLS[fill] >> 16
        else:
            assert int(want.view(torch.int32)) & 0xFFFFFFFF == P.FILLS[fill]
    assert a.intact()
    t = torch.arange(12, dtype=torch.float32).view(3, 4)
    p = a.place(t)
    assert p.shape == t.shape and torch.equal(p, t) and p.data_ptr() % 256 == 0 and a.intact()
    # a store one element past the operand, or one in front of it, is seen
    torch.as_strided(p, (1,), (1,), p.storage_offset() + 12).fill_(3.0)
    assert not a.intact()
    torch.as_strided(p, (1,), (1,), p.storage_offset() + 12).copy_(P.fill_(torch.empty(1), fill))
    assert a.intact()
    torch.as_strided(p, (1,), (1,), p.storage_offset() - 1).fill_(3.0)
    assert not a.intact()


def test_same_bits_reports_count_place_and_values():
    a = torch.tensor([[1.0, 2.0, float("nan")], [4.0, 5.0, 6.0]], dtype=torch.float16)
    b = a.clone()
    assert P.same_bits(a, b) is None                           # NaN against the same NaN: equal bits
    b[1, 0], b[1, 2] = 4.004, -6.0
    msg = P.same_bits(a, b)
    assert msg.startswith("2 of 6 elements differ, the first at (row 1, column 0)") and "0x4400" in msg and "0x4401" in msg
    assert P.same_bits(torch.tensor([0.0]), torch.tensor([-0.0])) is not None


def test_hooks_without_a_fill_allocate_as_before():
    be = ER.Hooks(None, {"w": torch.ones(4, 8)}, {"ids": torch.arange(6).view(2, 3)}, 256, "cpu")
    assert be.arena is None and be.buf["w"].shape == (4, 8) and be.buf["ids"].dtype == torch.int64
    for name, elems, kind in (("x", 10, "f16"), ("stats", 7, "f32"), ("index", 3, "i32")):
        be.alloc(name, elems, kind)
        t = be.buf[name]
        assert t.numel() == elems + ER.Hooks.PAD == elems + 4096 and t.dtype == ER.Hooks.KINDS[kind] and not bool(t.count_nonzero())
    first = be.buf["x"]
    be.alloc("x", 10)
    assert be.buf["x"] is first
    be.alloc("x", 11)
    assert be.buf["x"] is not first and be.buf["x"].numel() == 11 + 4096


@pytest.mark.parametrize("fill", list(P.FILLS))
def test_hooks_with_a_fill_guard_every_buffer(fill):
    w = {"c_fc.bias": torch.full((48,), 0.5), "c_fc.weight": torch.full((48, 12), 0.25, dtype=torch.float16)}
    ids = torch.arange(6).view(2, 3)
    be = ER.Hooks(None, w, {"ids": ids}, 256, "cpu", fill=fill)
    assert be.arena.fill == fill and be.arena.guard == 256 * 48 > ER.Hooks.PAD          # one 256-row tile of the widest row
    assert torch.equal(be.buf["c_fc.weight"], w["c_fc.weight"]) and torch.equal(be.buf["ids"], ids) and be.buf["ids"].dtype == torch.int64
    be.alloc("x", 10)
    be.alloc("index", 3, "i32")
    assert be.buf["x"].numel() == 10 and be.buf["index"].numel() == 3
    assert P.same_bits(be.buf["x"], P.fill_(torch.empty(10, dtype=torch.float16), fill)) is None
    assert be.buf["index"].tolist() == [P.int_fill(fill)] * 3
    be._table([0, 3, 5])
    assert be.keep[-1].tolist() == [0, 3, 5] and len(be.arena.keep) == 6
    assert all(t.data_ptr() % 256 == 0 for t in list(be.buf.values()) + be.keep) and be.arena.intact()
    for i in range(len(be.arena.keep)):
        assert all(g.numel() >= be.arena.guard for g in be.arena.guards(i))
    # weights guarded once by the caller (shared among replays) are used as they are; inputs and scratch get the same guard
    placed = P.Arena(fill, "cpu", P.guard_elems(ER.Hooks.widest_row(w))).place_all(w)
    shared = ER.Hooks(None, placed, {"ids": ids}, 256, "cpu", fill=fill)
    assert all(shared.buf[k] is placed[k] for k in w) and shared.arena.guard == placed.arena.guard == 256 * 48
    assert len(shared.arena.keep) == 1 and torch.equal(shared.buf["ids"], ids) and len(placed.arena.keep) == 2 and placed.arena.intact()
    with pytest.raises(AssertionError):
        ER.Hooks(None, placed, {}, 256, "cpu", fill="zero" if fill != "zero" else "big")


# ---- three emulations of a tiled kernel, each clean and with one planted defect -------------------------------------------------------

TILE = 8


def _window(t, rows, cols, ld, off=0):
    """rows x cols elements of the memory t lies in, from its element `off` on with row stride ld: a kernel's view, past the operand's
    end where the shape says so."""
    return torch.as_strided(t, (rows, cols), (ld, 1), t.storage_offset() + off)


def emu_row_sums(arena, x, defect):
    """Row sums of fp16 x [M, N] in tiles of TILE columns, fp32 accumulation.  The last tile of a row reaches past column N -- into the
    next row, and for the last row past the operand.  Clean: the tail is SELECTED away.  Defect: it is multiplied by 0."""
    M, N = x.shape
    mem = arena.place(x)
    out = arena.take(M, "f32")
    acc = torch.zeros(M)
    for c0 in range(0, N, TILE):
        v = _window(mem, M, TILE, N, c0).float()
        live = (c0 + torch.arange(TILE) < N)[None]
        acc = acc + (v * live.float() if defect else torch.where(live, v, torch.zeros(()))).sum(dim=1)
    out.copy_(acc)
    return out.clone()


def emu_lazy_softmax(arena, q, k, v, Lq, defect):
    """Rows [0, Lq) of softmax(q k^T) v for fp16 q [L, d] with the LAZY reference of the attention kernels: one tile of TILE query rows,
    keys in blocks of TILE; the reference m only moves when SOME row of the tile has a block maximum above m + 8, and then every row
    moves to its own maximum.  The tile's spare rows (>= Lq) are loaded too.  Clean: a spare row repeats row Lq - 1.  Defect: it is
    row min(r, L - 1) of the buffer -- a Q slot the caller never wrote where only the first Lq were projected."""
    L, d = k.shape
    assert Lq <= TILE <= L
    qmem = arena.take(L * d, "f16").view(L, d)
    qmem[:Lq].copy_(q[:Lq])                                   # only the first Lq query rows are ever written
    kk, vv = arena.place(k).float(), arena.place(v).float()
    out = arena.take(Lq * d, "f32")
    rows = torch.arange(TILE).clamp(max=(L if defect else Lq) - 1)
    qt = qmem[rows].float()
    m = torch.full((TILE,), float("-inf"))
    l, o = torch.zeros(TILE), torch.zeros(TILE, d)
    for k0 in range(0, L, TILE):
        s = qt @ kk[k0:k0 + TILE].t()
        mx = torch.where(torch.isnan(s), torch.full((), float("-inf")), s).max(dim=1).values      # fmaxf: a NaN operand loses
        mx = torch.where(torch.isnan(s).all(dim=1), torch.full((), float("nan")), mx)
        if bool((mx > m + 8.0).any()):                         # the ballot: NaN > x is false
            m_new = torch.where(mx > m, mx, m)                 # fmaxf(m, mx)
            alpha = torch.exp2(m - m_new)
            l, o, m = l * alpha, o * alpha[:, None], m_new
        p = torch.exp2(s - m[:, None]).half().float()
        l, o = l + p.sum(dim=1), o + p @ vv[k0:k0 + TILE]
    out.view(Lq, d).copy_((o / l[:, None])[:Lq])
    return out.clone()


def emu_accumulate(arena, a, b, defect):
    """C = A B^T in fp32, K in steps of TILE.  Clean: the accumulator starts at zero.  Defect: it starts as whatever the output buffer
    holds (a kernel that accumulates into memory it assumes zero)."""
    A, B = arena.place(a), arena.place(b)
    out = arena.take(a.shape[0] * b.shape[0], "f32").view(a.shape[0], b.shape[0])
    acc = out.clone() if defect else torch.zeros_like(out)
    for k0 in range(0, a.shape[1], TILE):
        acc = acc + A[:, k0:k0 + TILE].float() @ B[:, k0:k0 + TILE].float().t()
    out.copy_(acc)
    return out.clone()


def _operands():
    g = torch.Generator().manual_seed(3)
    x = torch.randn((5, 13), generator=g).half()
    L, d, Lq = 24, 16, 1
    # row 0 = e_0 sees column 0 of k alone: scores of about +-0.5, and 3.3 at key 13 -- the second block lifts row 0's maximum by less
    # than 8, so on its own row 0 keeps its reference.  Column 1 (that row 0 does not see) grows by 8 per block: a spare row that holds
    # anything positive asks for a move in every block.
    v = torch.randn((L, d), generator=g).half()
    q, k = torch.zeros((L, d), dtype=torch.float16), torch.zeros((L, d), dtype=torch.float16)
    q[0, 0] = 1.0
    k[:, 0] = (0.5 * torch.randn(L, generator=g)).half()
    k[13, 0] = 3.3
    k[:, 1] = (8 * (torch.arange(L) // TILE)).half()
    a, b = torch.randn((6, 24), generator=g).half(), torch.randn((7, 24), generator=g).half()
    return {"tail": lambda ar, bad: emu_row_sums(ar, x, bad),
            "vote": lambda ar, bad: emu_lazy_softmax(ar, q, k, v, Lq, bad),
            "accumulator": lambda ar, bad: emu_accumulate(ar, a, b, bad)}


DETECTS = {                     # defect -> the fills under which its output differs from the one under `zero`
    "tail": {"nan16": True, "ones": True, "big": False},
    "vote": {"nan16": False, "ones": False, "big": True},
    "accumulator": {"nan16": True, "ones": True, "big": True},
}


def test_detection_matrix():
    emus = _operands()
    assert set(emus) == set(DETECTS)
    got = {}
    for name, run in emus.items():
        clean = {f: run(P.Arena(f, "cpu", P.guard_elems(24)), False) for f in P.FILLS}
        assert bool(torch.isfinite(clean["zero"]).all()), name
        for f in NONZERO:
            assert P.same_bits(clean[f], clean["zero"]) is None, f"the clean '{name}' emulation depends on the fill {f}: {P.same_bits(clean[f], clean['zero'])}"
        bad = {f: run(P.Arena(f, "cpu", P.guard_elems(24)), True) for f in P.FILLS}
        # over clean memory the defect does not show: what every other suite hands the kernels
        assert P.same_bits(bad["zero"], clean["zero"]) is None, name
        got[name] = {f: P.same_bits(bad[f], bad["zero"]) is not None for f in NONZERO}
    assert got == DETECTS, got
    # no single fill sees all three defects: `big` misses the tail, the NaN fills miss the vote
    for f in NONZERO:
        assert not all(DETECTS[d][f] for d in DETECTS)
    assert all(any(DETECTS[d][f] for f in NONZERO) for d in DETECTS)


def test_vote_defect_needs_a_move_inside_the_threshold():
    """Why the `vote` operands spike a key: without a block maximum of row 0 between m and m + 8 the forced move changes nothing."""
    g = torch.Generator().manual_seed(3)
    L, d = 24, 16
    q, v = torch.randn((L, d), generator=g).half(), torch.randn((L, d), generator=g).half()
    k = torch.zeros((L, d), dtype=torch.float16)               # every score 0: the reference never has a reason to move
    outs = [emu_lazy_softmax(P.Arena(f, "cpu", P.guard_elems(24)), q, k, v, 1, True) for f in ("zero", "big")]
    assert P.same_bits(outs[0], outs[1]) is None


# ---- which cases test_hip_poison.py replays over guarded operands, and which head shapes it runs -----------------------------------------

def test_hook_cases_cover_every_family_and_kernel():
    import test_hip_poison as T
    chosen = T.hook_cases()
    assert len(chosen) == len(set(chosen))
    assert {T._family(ER.BY_NAME[n]) for n in chosen} == {T._family(c) for c in ER.CASES}
    assert {f for _, f in (T._family(c) for c in ER.CASES)} == {"tiny", "small", "b16", "head768"}
    assert set().union(*(T._kernels(ER.BY_NAME[n]) for n in chosen)) == set().union(*(T._kernels(c) for c in ER.CASES))
    hooks = {k[0] for n in chosen for k in T._kernels(ER.BY_NAME[n])}
    assert hooks >= {"gemm", "gemm_patches", "gemm_strided", "lnfold", "layernorm", "attention", "attention_q", "attention_f32_varlen",
                     "attention_f32_long", "l2norm", "text_ensemble", "text_embed_ids", "text_add_pos", "gather_rows", "im2col", "fill_cls"}


def test_head_shapes_reach_every_instantiation_on_256_cus():
    import head_exact as H
    import test_hip_poison as T
    assert T.head_shapes(256) == T.HEAD_SHAPES and all(s in H.SHAPES for s in T.HEAD_SHAPES)
    H.assert_coverage(T.HEAD_SHAPES, 256)
    for n_cu in (64, 120):                                     # smaller devices: the list reaches, or grows until it reaches, every instantiation
        H.assert_coverage(T.head_shapes(n_cu), n_cu)


# ---- the hook, without a GPU ------------------------------------------------------------------------------------------------------------

def test_fill_workspace_hook_is_declared_exported_and_checks_its_handle():
    from ovmr_amd import build, runtime
    text = open(os.path.join(REPO, "include", "ovmr_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int ovmr_debug_fill_workspace\(ovmr_handle\* h, uint32_t pattern, ovmr_stream stream\);", text, re.S)
    assert m, "ovmr_debug_fill_workspace is not declared in include/ovmr_hip.h"
    words = " ".join(m.group(1).replace("*", " ").split())
    for needle in ("hipMemsetD32Async", "allocates nothing", "does not synchronise", "OVMR_E_ARG for a NULL handle", "OVMR_E_STATE before ovmr_finalize",
                   "never touches", "spin forever"):
        assert needle in words, needle
    assert runtime.SIGNATURES["ovmr_debug_fill_workspace"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p])
    if not os.path.exists(runtime.LIB_PATH):
        build.build(verbose=False)
    lib = runtime.load_library()
    assert hasattr(lib, "ovmr_debug_fill_workspace")
    assert lib.ovmr_debug_fill_workspace(None, 0x7E007E00, None) == -1          # OVMR_E_ARG: nothing launched, no GPU needed
    import boundary_cases as bc
    assert "ovmr_debug_fill_workspace" in bc.EXEMPT
