"""The row kernels between the GEMMs held to exact values (rowops_exact.py: the three methods, the operands, the derivation of the
LayerNorm budget; test_rowops_exact_cpu.py: honest evaluations pass, each planted defect is rejected).

  * layernorm_rows through ovmr_debug_layernorm: every case of rowops_exact.LN_CASES out of place, in place (y == x) and with
    in_stride = D + 4 and 2 D (the gap columns filled with NaN) -- decided bits under the derived budget E (fp16), |got - out| <= E
    (fp32), constant rows equal to beta bit for bit; an out-of-place launch leaves its input as it was;
  * l2norm_f16_kernel through ovmr_debug_l2norm, once and twice: the "exact" set has ONE bit pattern per element, arbitrary fp16 rows
    equal, as whole rows, the row computed with one of at most two candidate norms per application; the all-zero row stays zero and the
    row whose norm overflows fp16 gives signed zeros;
  * the prompt ensemble through ovmr_debug_text_ensemble: both vector kernels, the element-wise kernel at widths they do not take and,
    at E = 512, behind an `out` that is 2-byte aligned only -- where it must agree bit for bit with the vector kernel;
  * the text front through ovmr_debug_text_embed_ids / _text_add_pos / _gather_rows on tables that carry their own row and column,
    ovmr_embed_tokens and ovmr_assemble_prompts through an engine on the tiny spec whose token table is such a table: bit equality.

Every output sits between rowops_exact.GUARD guard rows that must come back untouched.  The last test prints, per LayerNorm case, the
undecided share, the worst err / E of the two CPU evaluations and the worst err / E the device's output shows (the table in
rowops_exact.py).  Needs an MI355X: run with `pytest -m gpu`.
"""
import ctypes

import pytest
import torch

import gemm_exact as G
import rowops_exact as R
from conftest import usable_threads

pytestmark = pytest.mark.gpu

_LN_FIGURES = {}
_L2_FIGURES = {}


@pytest.fixture(scope="module")
def lib():
    from ovmr_amd import runtime
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    torch.set_num_threads(usable_threads())
    return runtime.load_library()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _back(buf, rows, what):
    """The guarded buffer back on the host: its guards checked, its middle rows returned."""
    torch.cuda.synchronize()
    host = buf.cpu()
    msg = R.guards_untouched(host, rows)
    assert msg is None, f"{what}: {msg}"
    return host[R.GUARD:R.GUARD + rows]


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------

def _ln_launch(lib, c, ops, mode, gd, bd, what):
    rows, D = c.rows, c.D
    dt = torch.float32 if c.f32 else torch.float16
    stride = {"out_of_place": D, "in_place": D, "stride_d+4": D + 4, "stride_2d": 2 * D}[mode]
    buf, y = R.guarded(rows, D, dt, "cuda")
    if mode == "in_place":
        y.copy_(ops.x)
        xin = y
    else:
        xin = torch.full((rows, stride), float("nan"), dtype=dt, device="cuda")
        xin[:, :D] = ops.x.cuda()
        before = xin.clone()
    assert xin.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
    rc = lib.ovmr_debug_layernorm(int(c.f32), _p(xin), _p(y), _p(gd), _p(bd), rows, D, stride, _s())
    assert rc == 0, f"{what}: rc {rc}"
    got = _back(buf, rows, what)
    if mode != "in_place":
        assert torch.equal(G.bits(xin), G.bits(before)), f"{what}: the input was written"
    return got


@pytest.mark.parametrize("c", R.LN_CASES, ids=lambda c: c.id)
def test_layernorm_exact(lib, c):
    und_n = und_d = 0
    worst = {"kernel": 0.0, "torch": 0.0, "device": 0.0}
    for row0 in R.ln_row0s(c.rows):
        ops = R.ln_operands(c, row0)
        ref = R.ln_reference(ops)
        ordinary = ~ops.const
        if bool(ordinary.any()):
            und = (G.bits(ref.lo) != G.bits(ref.hi))[ordinary]
            und_n, und_d = und_n + int(und.sum()), und_d + und.numel()
            assert R.ln_undecided_share(ref) <= R.MAX_UNDECIDED
            for order in ("kernel", "torch"):
                err = (R.ln_emulate(ops, order).double() - ref.x).abs()
                worst[order] = max(worst[order], float(R.over_E(err, ref.E)[ordinary].max()))
        gd, bd = ops.g.cuda(), ops.b.cuda()
        first = None
        for mode in R.LN_MODES:
            what = f"{c.id}, row 0 {row0}, {mode}"
            got = _ln_launch(lib, c, ops, mode, gd, bd, what)
            worst["device"] = max(worst["device"], R.ln_observed(got, ref))
            msg = R.ln_mismatch(got, ref)
            assert msg is None, f"{what}: {msg}"
            if first is None:
                first = got
            assert torch.equal(G.bits(got), G.bits(first)), f"{what}: differs from the out-of-place launch"
    _LN_FIGURES[c.id] = (und_n / max(und_d, 1), worst["kernel"], worst["torch"], worst["device"])


def test_layernorm_argument_errors(lib):
    x = torch.zeros((4, 2052), dtype=torch.float16, device="cuda")
    g = torch.ones(2052, device="cuda")
    for D, stride in ((6, 6), (2052, 2052), (64, 66)):
        assert lib.ovmr_debug_layernorm(0, _p(x), _p(x), _p(g), _p(g), 4, D, stride, _s()) == -2


# ---- L2 norm -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", R.L2_D)
@pytest.mark.parametrize("rows", R.L2_ROWS)
def test_l2norm_exact(lib, rows, D):
    two = 0.0
    for kind in R.L2_SETS:
        for row0 in R.l2_row0s(rows):
            X, pinned = R.l2_operands(rows, D, kind, row0)
            exact = ~pinned if kind == "exact" else False
            for times in (1, 2):
                what = f"l2-{rows}x{D}-{kind}-x{times}, row 0 {row0}"
                buf, y = R.guarded(rows, D, torch.float16, "cuda")
                y.copy_(X)
                rc = lib.ovmr_debug_l2norm(_p(y), rows, D, times, _s())
                assert rc == 0, f"{what}: rc {rc}"
                got = _back(buf, rows, what)
                cands = R.l2_candidates(X, times, exact)
                two = max(two, R.two_norm_share(cands))
                if kind == "exact" and times == 1:                        # ONE bit pattern
                    msg = G.bits_mismatch(got, cands[0])
                else:
                    msg = R.rows_mismatch(got, cands)
                assert msg is None, f"{what}: {msg}"
                for row, pin in R.l2_pins(rows, row0).items():
                    want = X[row] if pin == "zero" else torch.copysign(torch.zeros(D), X[row].float()).half()
                    assert torch.equal(G.bits(got[row]), G.bits(want)), f"{what}: the {pin} row {row}"
    _L2_FIGURES[(rows, D)] = two


def test_l2norm_argument_errors(lib):
    x = torch.zeros((4, 64), dtype=torch.float16, device="cuda")
    assert lib.ovmr_debug_l2norm(_p(x), 4, 6, 1, _s()) == -1
    assert lib.ovmr_debug_l2norm(None, 4, 64, 1, _s()) == -1
    assert lib.ovmr_debug_l2norm(_p(x), 4, 64, 0, _s()) == 0 and lib.ovmr_debug_l2norm(_p(x), 0, 64, 1, _s()) == 0


# ---- prompt ensemble ---------------------------------------------------------------------------------------------------------------

def _ensemble(lib, feats_d, T, rows, E, what, misalign=False):
    """One launch; `misalign`: `out` one element behind a 16-byte boundary, in a flat guarded buffer."""
    n = rows * E
    flat = G.sentinel_buffer(1, n + 2 * R.GUARD * E + 8, torch.float16, "cuda")[0]
    start = R.GUARD * E + (1 if misalign else 0)
    out = flat[start:start + n]
    assert feats_d.data_ptr() % 16 == 0 and out.data_ptr() % 16 == (2 if misalign else 0)
    rc = lib.ovmr_debug_text_ensemble(_p(feats_d), T, rows, E, _p(out), _s())
    assert rc == 0, f"{what}: rc {rc}"
    torch.cuda.synchronize()
    host = flat.cpu()
    b = G.bits(host)
    assert bool((b[:start] == G.SENTINEL).all()) and bool((b[start + n:] == G.SENTINEL).all()), f"{what}: wrote outside the output"
    return host[start:start + n].view(rows, E).clone()


@pytest.mark.parametrize("E", R.ENS_E_V8 + R.ENS_E_ANY)
@pytest.mark.parametrize("T", R.ENS_T)
def test_text_ensemble_exact(lib, T, E):
    for rows in R.ENS_ROWS:
        feats = R.ens_operands(T, rows, E)
        cands, _ = R.ens_reference(feats)
        fd = feats.cuda()
        kernel = "v8<1>" if E in R.ENS_E_V8 and E <= 512 else "v8<2>" if E in R.ENS_E_V8 else "any"
        what = f"ens-T{T}-{rows}x{E} ({kernel})"
        got = _ensemble(lib, fd, T, rows, E, what)
        msg = R.rows_mismatch(got, cands)
        assert msg is None, f"{what}: {msg}"
        if E == 512:                                                      # the element-wise kernel behind a 2-byte aligned `out`
            other = _ensemble(lib, fd, T, rows, E, what + ", out 2-byte aligned (any)", misalign=True)
            msg = R.rows_mismatch(other, cands)
            assert msg is None, f"{what}, out 2-byte aligned (any): {msg}"
            msg = G.bits_mismatch(other, got)
            assert msg is None, f"{what}: the element-wise and the vector kernel disagree: {msg}"


def test_text_ensemble_argument_errors(lib):
    x = torch.zeros(1024, dtype=torch.float16, device="cuda")
    assert lib.ovmr_debug_text_ensemble(_p(x), 0, 2, 8, _p(x), _s()) == -1
    assert lib.ovmr_debug_text_ensemble(_p(x), 1, 2, 0, _p(x), _s()) == -1
    assert lib.ovmr_debug_text_ensemble(None, 1, 2, 8, _p(x), _s()) == -1
    assert lib.ovmr_debug_text_ensemble(_p(x), 1, 0, 8, _p(x[512:]), _s()) == 0


# ---- text front --------------------------------------------------------------------------------------------------------------------

_INDEX_GUARD = -77


@pytest.mark.parametrize("D", R.TEXT_D)
@pytest.mark.parametrize("Lseq", R.TEXT_LSEQ)
@pytest.mark.parametrize("N", R.TEXT_N)
def test_text_front_exact(lib, N, Lseq, D):
    tok, pos, prm = R.tok_table(D), R.pos_table(D), R.prompt_table(N, D)
    tokd, posd, prmd = tok.cuda(), pos.cuda(), prm.cuda()
    rows = N * Lseq
    for stride in R.TEXT_STRIDES:
        what = f"text-{N}x{Lseq}x{D}, ids_stride {stride}"
        ids = R.ids_table(N, stride)
        want_x, want_index = R.embed_ids_reference(ids, tok, pos, Lseq)
        buf, x = R.guarded(rows, D, torch.float16, "cuda")
        index = torch.full((N + 2 * R.GUARD,), _INDEX_GUARD, dtype=torch.int32, device="cuda")
        idsd = ids.cuda()                                                 # (named: a temporary's memory is free again before the launch)
        rc = lib.ovmr_debug_text_embed_ids(_p(idsd), stride, _p(tokd), _p(posd), _p(x), _p(index[R.GUARD:]), N, R.LCTX, Lseq, D, _s())
        assert rc == 0, f"{what}: rc {rc}"
        got = _back(buf, rows, what)
        msg = G.bits_mismatch(got, want_x)
        assert msg is None, f"{what}, text_embed_ids_kernel (row = sequence * {Lseq} + position): {msg}"
        idx = index.cpu()
        assert bool((idx[:R.GUARD] == _INDEX_GUARD).all()) and bool((idx[R.GUARD + N:] == _INDEX_GUARD).all()), f"{what}: index guards"
        assert torch.equal(idx[R.GUARD:R.GUARD + N], want_index), f"{what}, argmax_ids_kernel: got {idx[R.GUARD:R.GUARD + N].tolist()}, want {want_index.tolist()}"
    # the positional add of embedded prompts
    what = f"text-{N}x{Lseq}x{D}"
    buf, x = R.guarded(rows, D, torch.float16, "cuda")
    rc = lib.ovmr_debug_text_add_pos(_p(prmd), R.LCTX, _p(posd), _p(x), N, Lseq, D, _s())
    assert rc == 0, f"{what}: rc {rc}"
    msg = G.bits_mismatch(_back(buf, rows, what), R.add_pos_reference(prm, pos, Lseq))
    assert msg is None, f"{what}, text_add_pos_kernel: {msg}"
    # the gather: the argmax of the ids (past Lseq where the sequence is cut short) and indices outside [0, Lseq) on both sides
    xd = want_x.cuda()
    for index in (want_index, R.gather_indices(N, Lseq)):
        buf, out = R.guarded(N, D, torch.float16, "cuda")
        indexd = index.cuda()
        rc = lib.ovmr_debug_gather_rows(_p(xd), _p(indexd), _p(out), N, Lseq, D, _s())
        assert rc == 0, f"{what}: rc {rc}"
        msg = G.bits_mismatch(_back(buf, N, what), R.gather_reference(want_x, index, Lseq))
        assert msg is None, f"{what}, gather_rows_kernel with index {index.tolist()}: {msg}"


def test_text_front_argument_errors(lib):
    x = torch.zeros(4096, dtype=torch.float16, device="cuda")
    i = torch.zeros(64, dtype=torch.int64, device="cuda")
    f = torch.zeros(4096, dtype=torch.float32, device="cuda")
    n = torch.zeros(8, dtype=torch.int32, device="cuda")
    assert lib.ovmr_debug_text_embed_ids(_p(i), 8, _p(f), _p(x), _p(x), _p(n), 1, 8, 9, 64, _s()) == -1      # Lseq > Lctx
    assert lib.ovmr_debug_text_embed_ids(_p(i), 7, _p(f), _p(x), _p(x), _p(n), 1, 8, 8, 64, _s()) == -1      # ids_stride < Lctx
    assert lib.ovmr_debug_text_embed_ids(_p(i), 8, _p(f), _p(x), _p(x), _p(n), 1, 8, 8, 6, _s()) == -1       # D % 4
    assert lib.ovmr_debug_text_add_pos(_p(x), 8, _p(x), _p(x), 1, 9, 64, _s()) == -1
    assert lib.ovmr_debug_gather_rows(_p(x), None, _p(x), 1, 8, 64, _s()) == -1
    assert lib.ovmr_debug_gather_rows(_p(x), _p(n), _p(x), 0, 8, 64, _s()) == 0


_ENGINES = {}


def _engine(n_ctx):
    """An engine on the tiny spec whose token table is rowops_exact.tok_table: one per n_ctx, shared by the tests."""
    from ovmr_amd import modules, synth
    if n_ctx not in _ENGINES:
        spec = synth.SPECS["tiny"]
        sd = {k: torch.from_numpy(v) for k, v in synth.clip_state_dict(spec, 11, jitter=True).items()}
        sd["token_embedding.weight"] = R.tok_table(spec.transformer_width, spec.vocab_size)
        e = modules.CLIPModel(sd, spec).engine(n_ctx)
        e.load_state_dict({}, {k: torch.from_numpy(v) for k, v in synth.prompt_learner_state_dict(spec, n_ctx, 11, True).items()})
        e.finalize(8, 8, 8)
        _ENGINES[n_ctx] = (e, spec)
    return _ENGINES[n_ctx]


@pytest.mark.parametrize("n_ctx", (1, 2))
def test_embed_tokens_and_assemble_prompts_exact(lib, n_ctx):
    e, spec = _engine(n_ctx)
    D, Lctx = spec.transformer_width, spec.context_length
    assert Lctx == R.LCTX and spec.embed_dim == D
    tok = R.tok_table(D, spec.vocab_size)
    gen = torch.Generator().manual_seed(n_ctx)
    for N, L in ((1, 1), (3, 9), (5, Lctx)):                              # N * L rows: 1, 27 and 385, none a multiple of 4
        what = f"embed_tokens {N}x{L}, n_ctx {n_ctx}"
        ids = torch.randint(0, spec.vocab_size, (N, L), generator=gen)
        ids[0, 0], ids[-1, -1] = spec.vocab_size - 1, 0
        buf, out = R.guarded(N * L, D, torch.float16, "cuda")
        idsd = ids.cuda()
        rc = lib.ovmr_embed_tokens(e.h, _p(idsd), N, L, _p(out), _s())
        assert rc == 0, f"{what}: rc {rc}"
        msg = G.bits_mismatch(_back(buf, N * L, what), R.embed_tokens_reference(ids, tok).view(N * L, D))
        assert msg is None, f"{what}, embed_gather_kernel: {msg}"
    base = R.prompt_table(6, D)
    based = base.cuda()
    for Cb in (1, 5):
        tokens = tok[torch.randint(0, spec.vocab_size, (Cb * n_ctx,), generator=gen)].view(Cb, n_ctx, D).contiguous()
        for labels in (torch.tensor([3, 0, 5, 5, 1][:Cb]), None):
            what = f"assemble_prompts Cb {Cb}, n_ctx {n_ctx}, labels {None if labels is None else labels.tolist()}"
            buf, out = R.guarded(Cb * Lctx, D, torch.float16, "cuda")
            labelsd, tokensd = None if labels is None else labels.cuda(), tokens.cuda()
            rc = lib.ovmr_assemble_prompts(e.h, _p(based), _p(labelsd), _p(tokensd), Cb, _p(out), _s())
            assert rc == 0, f"{what}: rc {rc}"
            msg = G.bits_mismatch(_back(buf, Cb * Lctx, what), R.assemble_reference(base, labels, tokens, n_ctx).reshape(Cb * Lctx, D))
            assert msg is None, f"{what}, assemble_prompts_kernel (row = class * {Lctx} + position): {msg}"


# ---- report ------------------------------------------------------------------------------------------------------------------------

def test_report_figures():
    """Prints the "Measured" table of rowops_exact.py for the cases run in this session: per LayerNorm case the undecided share, the
    worst err / E of the two CPU evaluations (kernel order, torch order) and the worst err / E the device's output shows; per L2 shape
    the largest share of rows with two candidate rows."""
    for cid, (share, k, t, dev) in _LN_FIGURES.items():
        print(f"\n    {cid:22s} undecided {share:6.2%}   err / E {k:.3f} {t:.3f}   MI355X {dev:.3f}")
    for (rows, D), two in _L2_FIGURES.items():
        print(f"\n    l2-{rows}x{D:<16d} rows with two candidates, at most {two:6.2%}")
