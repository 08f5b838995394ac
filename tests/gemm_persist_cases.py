"""Cases, operands and a CPU model of the tile loop of the LayerNorm-folding ping-pong GEMMs (ovmr_amd/csrc/gemm_f16_v5.hip, "Tile
loop").  Plain torch, no library: shared by test_hip_gemm_persist_cases.py (GPU) and test_gemm_persist_cases_cpu.py, which proves on the
CPU that the table reaches what it claims and that the comparator rejects the tile-loop defects it is there for.

Operands, reference and comparator are gemm_ln_exact's (columns, row_sums, reference, ln_mismatch, MAX_UNDECIDED) and gemm_exact's (_aw,
product, sentinel_buffer, outside_untouched, bits_mismatch); row_sums indexes row 259, so M >= 261.  The statistics are split over the
slots by slot_split here (below), for any slot count independent of K: ovmr_debug_gemm_persist takes ln_slots from the caller.

The table, (M, N, K, slots):
    785 x  576 x  256, 1     4 x 3 tiles   ragged N: the last N tile has 64 columns
    785 x  448 x  768, 3     4 x 2         the last N tile has 192 columns; a production width
    785 x 2304 x  256, 1     4 x 9         n_group = 4: groups of 4 + 4 + 1 N tiles, the fewest tiles that give them
    768 x  512 x 1024, 4     3 x 2         no guarded row tile; four slots, the last count the early load covers
    261 x  512 x  256, 5     2 x 2         exactly one late slot; the last row tile has 5 rows: 251 statistics rows of the prefetch clamped
    785 x  768 x 2048, 8     4 x 3         four late slots (slots = K / 256 as the engine sets it); 32 K-tiles
    785 x  576 x 1024, 6     4 x 3         late slots on guarded column tiles
   8200 x 3072 x  256, 1    33 x 12 = 396  the store hint (M N 2 >= 48 MiB), g4, more tiles than CUs: gemm_ln_exact's shape
  10989 x 2304 x  256, 1    43 x 9 = 387   the store hint with the short last group
Epilogue 6 on every case; epilogue 7 in both QuickGELU forms (variants 8 and 108) on 785 x 576 x 256 and on both hinted cases (forms_of).
Grids: 1, 2, 5, 7, tiles - 1, tiles; the hinted cases also 3, 255 and the production launch (max_wgs = 0, persist = 1: one workgroup per
CU, PRODUCTION = 256 in the model).  K = 1280 and K = 1536 are not in the table: their undecided share is 5.05 .. 5.21 %, above the cap.

Undecided share per case, in the table's order (asserted <= MAX_UNDECIDED = 5 % by the CPU test, which prints them):
    2.97 %  4.68 %  2.99 %  4.31 %  2.92 %  4.63 %  4.25 %  2.94 %  2.93 %

slot_split(su, sq, S): slot s >= 1 holds (+-(16 s + 1 + m % 7 + 8 (m // 256 % 2)) + 3/256, 32 s + 1 + m % 11 + 16 (m // 256 % 2) + 5/256), the
sign alternating with s, and slot 0 the rest.  The ranges of different slots are disjoint and the fractions keep slot 0 apart (3 S is no
multiple of 256), so for S > 1 every slot is non-zero and the slots of a row are pairwise distinct in both components; 256 = 4 mod 7 = 3
mod 11, so every slot s >= 1 differs between rows m and m +- 256; the odd slots' sums are negative.  Asserted there, with the usual: all
multiples of 2^-8, magnitudes summing below 2^16, the slots adding up to (su, sq).  (S = 1: the one slot is (su, sq), zero on row 3.)

The model.  walk(c, grid): workgroup w of min(grid, tiles) takes the dispatch slots w, w + grid, ..., slot -> tile by tile_of of
test_gemm_persist_route_cpu.py (which holds the library's walk to it).  emulate_walk(c, grid, defect) assembles the output buffer --
PAD_ROWS sentinel rows behind M, PAD_COLS = 256 sentinel columns behind N -- tile by tile in that order, every element h64 of the fp64
reference formula, and plants one defect: what ONE wrong line of the kernel would produce (DEFECTS).  The two hinted cases run the
model on the first two and last two rows of every row tile (model_rows), which contains every tile boundary.

coverage(): what some workgroup goes through between consecutive tiles, over the 60 (case, grid) pairs: how many pairs reach it, and the
first; asserted by test_gemm_persist_cases_cpu.py, which prints this table.
    tm alone                      22   785x576x256-s1, grid 2       tn alone                      22   785x576x256-s1, grid 1
    tm and tn                     42   785x576x256-s1, grid 1       guarded -> guarded            14   785x576x256-s1, grid 1
    interior -> guarded row       30   785x576x256-s1, grid 2       guarded row -> interior       25   785x576x256-s1, grid 2
    interior -> guarded column     8   785x576x256-s1, grid 1       guarded column -> interior     9   785x576x256-s1, grid 1
    only tile guarded             26   785x576x256-s1, grid 7       last tile interior            39   785x576x256-s1, grid 1
    one tile beside several       17   785x576x256-s1, grid 7       corner not first              12   785x576x256-s1, grid 1
"guarded" is either direction; "corner": the tile guarded in both, as a workgroup's second or later tile; "only tile guarded": a one-tile
workgroup whose tile is guarded; "last tile interior": a workgroup of several tiles that ends on an interior one.  The two hinted cases
together reach the eight lines that need neither a guarded column tile (they have none) nor two guarded tiles in a row: asserted too.

Seconds per GPU test on an MI355X: test_hip_gemm_persist_cases.py's docstring.
"""
import functools
from typing import NamedTuple

import torch

import gemm_exact as G
import gemm_ln_exact as L
from test_gemm_persist_route_cpu import tile_of

BM = BN = 256
PAD_COLS = 256                          # sentinel columns behind N: a guarded column tile overhangs N by up to 192
PRODUCTION = 256                        # the production launch in the model: one workgroup per CU of an MI355X
FORMS = {"ln": (G.EPI_LN_BIAS, 8), "lnqgelu": (G.EPI_LN_BIAS_QGELU, 8), "lnqgelu-one-rounding": (G.EPI_LN_BIAS_QGELU, 108)}


class Case(NamedTuple):
    M: int
    N: int
    K: int
    slots: int

    @property
    def id(self):
        return f"{self.M}x{self.N}x{self.K}-s{self.slots}"

    @property
    def tiles_m(self):
        return (self.M + BM - 1) // BM

    @property
    def tiles_n(self):
        return (self.N + BN - 1) // BN

    @property
    def tiles(self):
        return self.tiles_m * self.tiles_n

    @property
    def n_group(self):
        return 4 if self.tiles_n >= 8 else self.tiles_n

    @property
    def hinted(self):
        """The route sets the store hint: the production kernels <6, 8, 528> and <7, 8, 2576>."""
        return self.M * self.N * 2 >= 48 << 20


CASES = [Case(785, 576, 256, 1), Case(785, 448, 768, 3), Case(785, 2304, 256, 1), Case(768, 512, 1024, 4), Case(261, 512, 256, 5),
         Case(785, 768, 2048, 8), Case(785, 576, 1024, 6), Case(8200, 3072, 256, 1), Case(10989, 2304, 256, 1)]
TILES = ((4, 3), (4, 2), (4, 9), (3, 2), (2, 2), (4, 3), (4, 3), (33, 12), (43, 9))
HINTED = [c for c in CASES if c.hinted]
RAGGED_SMALL = CASES[0]                                                      # the small ragged-N case that also runs epilogue 7
STRIDED = CASES[6]                                                           # more than four slots, ragged N: the strided launch
# what test_hip_gemm_persist.py walks at K = 256: one slot, N a whole number of tiles
OLD_CASES = [Case(785, 512, 256, 1), Case(785, 768, 256, 1)]
OLD_GRIDS = (1, 2, 5, 1 << 20)


def forms_of(c):
    return tuple(FORMS) if c.hinted or c == RAGGED_SMALL else ("ln",)


def grids(c):
    """The capped grids of a case; for a hinted case PRODUCTION stands for the launch with max_wgs = 0 and persist = 1."""
    g = (1, 2, 5, 7, c.tiles - 1, c.tiles)
    return g + (3, 255, PRODUCTION) if c.hinted else g


def assert_table():
    assert tuple((c.tiles_m, c.tiles_n) for c in CASES) == TILES
    assert [c.id for c in HINTED] == ["8200x3072x256-s1", "10989x2304x256-s1"] and all(c.tiles > PRODUCTION for c in HINTED)
    assert all(c.M >= 261 and c.N % 64 == 0 and c.K % 128 == 0 for c in CASES)
    assert {c.slots for c in CASES} == {1, 3, 4, 5, 6, 8} and not any(c.K in (1280, 1536) for c in CASES)
    assert all(c.n_group == (4 if c.N in (2304, 3072) else c.tiles_n) for c in CASES)


# ---- operands ------------------------------------------------------------------------------------------------------------------

def slot_split(su, sq, S):
    """[M, S, 2] fp32: (su, sq) over S >= 1 slots (module docstring); every slot non-zero, a row's slots distinct, the slots from 1 on
    different between rows 256 apart, the odd slots' sums negative; exact in fp32 in any order (asserted)."""
    M = su.numel()
    m = torch.arange(M)
    tile = (m // 256) % 2
    st = torch.zeros((M, S, 2), dtype=torch.float64)
    for s in range(1, S):
        st[:, s, 0] = (-1.0) ** s * (16 * s + 1 + m % 7 + 8 * tile).double() + 3 / 256
        st[:, s, 1] = (32 * s + 1 + m % 11 + 16 * tile).double() + 5 / 256
    st[:, 0, 0] = su - st[:, 1:, 0].sum(1)
    st[:, 0, 1] = sq - st[:, 1:, 1].sum(1)
    assert bool((st * 256 == (st * 256).round()).all()) and float(st.abs().sum(1).max()) < 2 ** 16, "statistics partials are not exact in fp32"
    assert torch.equal(st.sum(1), torch.stack([su, sq], 1)) and torch.equal(st.float().double(), st)
    if S > 1:
        assert bool((st != 0).all()), "a zero slot"
        for s in range(S):
            for t in range(s + 1, S):
                assert bool((st[:, s] != st[:, t]).all()), f"slots {s} and {t} share a value on some row"
        assert bool((st[256:, 1:] != st[:-256, 1:]).all()), "a slot repeats 256 rows on"
        assert bool((st[:, 1::2, 0] < 0).all())
    return st.float()


class Problem(NamedTuple):
    A: torch.Tensor             # fp16 [M, K]
    W: torch.Tensor             # fp16 [N, K]
    g: torch.Tensor             # fp32 [N] ln_g
    b: torch.Tensor             # fp32 [N] ln_b
    stats: torch.Tensor         # fp32 [M, slots, 2]
    ref: L.Reference


@functools.lru_cache(maxsize=None)
def problem(c):
    """Operands and gemm_ln_exact's Reference of a case: computed once, never written."""
    A, W = G._aw(c.M, c.N, c.K, False)
    G.assert_exact(A, W, c.id)
    g, b = L.columns(c.N, c.M * 13 + c.N * 5 + c.K * 3 + 7)
    su, sq, deg, mean, var = L.row_sums(c.M, c.K)
    L.assert_rows_distinct(mean, var)
    return Problem(A, W, g, b, slot_split(su, sq, c.slots), L.reference(G.product(A, W), su, sq, g, b, c.K, deg))


# ---- the walk and what it reaches ---------------------------------------------------------------------------------------------

def walk(c, grid):
    """Per workgroup of a grid capped at `grid`: the (tm, tn) it computes, in order."""
    g = min(grid, c.tiles)
    return [[tile_of(s, c.tiles_m, c.tiles_n, c.n_group) for s in range(w, c.tiles, g)] for w in range(g)]


def guards(c, t):
    """(the tile holds rows behind M, columns behind N): the guarded form of the epilogue."""
    return (t[0] + 1) * BM > c.M, (t[1] + 1) * BN > c.N


REACHES = ("tm alone", "tn alone", "tm and tn", "interior -> guarded row", "guarded row -> interior", "interior -> guarded column",
           "guarded column -> interior", "guarded -> guarded", "only tile guarded", "last tile interior", "one tile beside several",
           "corner not first")


def coverage(cases=None):
    """name of REACHES -> the (case id, grid) pairs at which some workgroup goes through it, in the table's order."""
    out = {}
    for c in (CASES if cases is None else cases):
        for grid in grids(c):
            wgs = walk(c, grid)
            lens = {min(len(w), 2) for w in wgs}
            for w in wgs:
                hit = []
                kinds = [guards(c, t) for t in w]
                if len(w) == 1 and any(kinds[0]):
                    hit.append("only tile guarded")
                if len(w) > 1 and not any(kinds[-1]):
                    hit.append("last tile interior")
                if lens == {1, 2}:
                    hit.append("one tile beside several")
                if any(k == (True, True) for k in kinds[1:]):
                    hit.append("corner not first")
                for (p, q), (kp, kq) in zip(zip(w, w[1:]), zip(kinds, kinds[1:])):
                    hit.append("tm and tn" if p[0] != q[0] and p[1] != q[1] else "tm alone" if p[0] != q[0] else "tn alone")
                    for name, k in (("row", (True, False)), ("column", (False, True))):
                        if not any(kp) and kq == k:
                            hit.append(f"interior -> guarded {name}")
                        if kp == k and not any(kq):
                            hit.append(f"guarded {name} -> interior")
                    if any(kp) and any(kq):
                        hit.append("guarded -> guarded")
                for h in hit:
                    if (c.id, grid) not in out.setdefault(h, []):
                        out[h].append((c.id, grid))
    return out


# ---- the model -------------------------------------------------------------------------------------------------------------------

DEFECTS = {
    "col_consts_prev": "the column constants of the workgroup's previous tile (cb not toggled)",
    "row_consts_prev": "the row constants of its previous tile",
    "late_slots_current_rows": "slots 4 and up read from the rows of the tile whose epilogue runs instead of the next tile's",
    "late_slots_dropped": "slots 4 and up dropped on every tile but a workgroup's first",
    "acc_not_cleared": "accumulators not cleared between tiles",
    "a_rows_prev": "the A rows of the previous tile (source_rows not refreshed)",
    "w_rows_prev": "the W rows of the previous tile",
    "ktile0_prev": "K-tile 0 left over from the previous tile: k in [0, 64) of the product from the old tile (the counted wait's hazard)",
    "guard_cols_off": "a guarded tile stores its full 256 columns",
    "guard_rows_off": "a guarded tile stores its full 256 rows",
    "last_slot_skipped": "the last dispatch slot never computed",
    "step_grid_minus_1": "a workgroup steps by grid - 1: slots computed twice, as many at the end never",
}


def model_rows(c):
    """The rows the model runs on: all of them, or (M > 1024) the first two and last two of every row tile."""
    if c.M <= 1024:
        return torch.arange(c.M)
    r = [m for tm in range(c.tiles_m) for m in (tm * BM, tm * BM + 1, min(c.M, (tm + 1) * BM) - 2, min(c.M, (tm + 1) * BM) - 1)]
    return torch.tensor(sorted(set(r)))


@functools.lru_cache(maxsize=None)
def _honest(c):
    rows = model_rows(c)
    return rows, L.h64(problem(c).ref.x[rows])


def _tile_x(c, p, t, prev, loc, defect, carry):
    """fp64 (x [len(loc), 256], acc) of tile t on its local rows `loc` with `defect` planted; prev: the workgroup's tile before."""
    d = defect if prev is not None else None
    prev = prev if prev is not None else t
    rows, prows = (torch.clamp(tt[0] * BM + loc, max=c.M - 1) for tt in (t, prev))
    cols, pcols = (tt[1] * BN + torch.arange(BN) for tt in (t, prev))
    wrow, pwrow = (torch.clamp(x, max=c.N - 1) for x in (cols, pcols))
    A, W = p.A.double(), p.W
    a = A[prows if d == "a_rows_prev" else rows]
    w = W[pwrow if d == "w_rows_prev" else wrow].double()
    if d == "ktile0_prev":
        acc = a[:, 64:] @ w[:, 64:].t() + A[prows][:, :64] @ W[pwrow].double()[:, :64].t()
    else:
        acc = a @ w.t()
    if d == "acc_not_cleared":
        acc = acc + carry
    st = p.stats.double()
    early = prows if d == "row_consts_prev" else rows
    late = prows if d in ("row_consts_prev", "late_slots_current_rows") else rows
    s = st[early, :4].sum(1)
    if d != "late_slots_dropped":
        s = s + st[late, 4:].sum(1)
    mean, rstd, _, _ = L.row_terms(s[:, 0], s[:, 1], c.K)
    cc = pcols if d == "col_consts_prev" else cols
    inside = (cc < c.N).double()                                            # load_consts: zero behind N
    g, b = (v.double()[torch.clamp(cc, max=c.N - 1)] * inside for v in (p.g, p.b))
    return rstd[:, None] * (acc - mean[:, None] * g[None]) + b[None], acc


def emulate_walk(c, grid, defect=None):
    """The output buffer [rows + PAD_ROWS, N + PAD_COLS] (fp16; rows: model_rows) as the walk of a grid capped at `grid` leaves it."""
    assert defect is None or defect in DEFECTS
    p = problem(c)
    rows, honest = _honest(c)
    nr = rows.numel()
    buf = G.sentinel_buffer(nr + G.PAD_ROWS, c.N + PAD_COLS)
    g = min(grid, c.tiles)
    step = g - 1 if defect == "step_grid_minus_1" else g
    for w in range(g):
        prev = carry = None
        for i in range(len(range(w, c.tiles, g))):
            slot = w + i * step
            if defect == "last_slot_skipped" and slot == c.tiles - 1:
                continue
            t = tile_of(slot, c.tiles_m, c.tiles_n, c.n_group)
            sel = (rows // BM == t[0]).nonzero().flatten()
            n0, nc = t[1] * BN, min(BN, c.N - t[1] * BN)
            gr, gc = guards(c, t)
            planted = defect in DEFECTS and (prev is not None and defect not in ("guard_cols_off", "guard_rows_off", "last_slot_skipped", "step_grid_minus_1")
                                             or defect == "guard_cols_off" and gc or defect == "guard_rows_off" and gr)
            if not planted and defect != "acc_not_cleared":
                buf[sel, n0:n0 + nc] = honest[sel, n0:n0 + nc]
            else:
                loc, dst = rows[sel] - t[0] * BM, sel
                if defect == "guard_rows_off" and gr:                   # the rows behind M, as far as the buffer goes
                    extra = torch.arange(min(G.PAD_ROWS, (t[0] + 1) * BM - c.M))
                    loc, dst = torch.cat([loc, c.M - t[0] * BM + extra]), torch.cat([sel, nr + extra])
                if defect == "acc_not_cleared":                         # an accumulator belongs to a position of the tile: all 256 rows
                    x, carry = _tile_x(c, p, t, prev, torch.arange(BM), defect, carry)
                    x = x[loc]
                else:
                    x, _ = _tile_x(c, p, t, prev, loc, defect, None)
                if defect == "guard_cols_off" and gc:
                    nc = BN
                buf[dst, n0:n0 + nc] = L.h64(x[:, :nc])
            prev = t
    return buf


def verdict(c, buf):
    """None if the buffer of emulate_walk passes what the GPU test asks of a launch, else (how, message): "sentinel" (outside_untouched),
    "decided" (ln_mismatch with at least one decided element of an ordinary row failing) or "undecided"."""
    rows, _ = _honest(c)
    msg = G.outside_untouched(buf, rows.numel(), c.N)
    if msg is not None:
        return "sentinel", msg
    ref = problem(c).ref.rows(rows)
    got = buf[:rows.numel(), :c.N].contiguous()
    msg = L.ln_mismatch(got, ref)
    if msg is None:
        return None
    ok, decided = L._ok(got, ref)
    return ("decided" if bool((~ok & decided & ~ref.deg[:, None]).any()) else "undecided"), msg
