"""gemm_persist_cases.py held to its own claims, without a GPU:

  * the table is the stated one, every case keeps the 5 % cap on undecided elements, and the (case, grid) pairs take some workgroup through
    every transition of REACHES (coverage());
  * the honest model of the walk passes the comparator and the sentinel check on every (case, grid);
  * every planted defect of the tile loop (DEFECTS) is rejected on the (case, grid) pairs named here, by a decided element or by the
    sentinel check;
  * the defects that need more than four statistics slots or a ragged N PASS on the shapes test_hip_gemm_persist.py walks (one slot,
    N = 512 / 768) at every grid it uses: it is this table that catches them.
"""
import pytest

import gemm_exact as G
import gemm_ln_exact as L
import gemm_persist_cases as P

BY_ID = {c.id: c for c in P.CASES}


def test_the_table_and_its_coverage():
    P.assert_table()
    cov = P.coverage()
    print()
    for name in P.REACHES:
        print(f"    {name:28s} {len(cov.get(name, ())):3d}   " + ("%s, grid %d" % cov[name][0] if name in cov else "-"))
    missing = [n for n in P.REACHES if n not in cov]
    assert not missing, f"no (case, grid) takes a workgroup through: {missing}"
    assert sum(len(P.grids(c)) for c in P.CASES) == 60
    # the production kernels: everything that needs no guarded column tile
    hinted = P.coverage(P.HINTED)
    assert [n for n in P.REACHES if n not in hinted] == ["interior -> guarded column", "guarded column -> interior", "guarded -> guarded", "corner not first"]
    # what the older shapes cannot reach: a guarded column tile
    old = P.coverage(P.OLD_CASES)
    assert not [n for n in old if "column" in n or n == "corner not first"]


@pytest.mark.parametrize("c", P.CASES, ids=lambda c: c.id)
def test_cap_and_the_honest_walk(c):
    ref = P.problem(c).ref
    share = L.undecided_share(ref)
    print(f"\n{c.id}: undecided {share:.2%}")
    assert share <= L.MAX_UNDECIDED, f"{c.id}: {share:.2%} of the elements undecided"
    first = None
    for grid in P.grids(c):
        buf = P.emulate_walk(c, grid)
        assert P.verdict(c, buf) is None, f"{c.id}, {grid} workgroups: {P.verdict(c, buf)}"
        if first is None:
            first = buf
        assert G.bits_mismatch(buf, first) is None, f"{c.id}: the walk of {grid} workgroups leaves another buffer"


# defect -> the (case, grid) pairs that must reject it
REJECTED_BY = {
    "col_consts_prev": [("785x576x256-s1", 5), ("10989x2304x256-s1", P.PRODUCTION)],
    "row_consts_prev": [("785x576x256-s1", 5), ("261x512x256-s5", 1), ("8200x3072x256-s1", 255)],
    "late_slots_current_rows": [("261x512x256-s5", 1), ("785x768x2048-s8", 5), ("785x576x1024-s6", 2)],
    "late_slots_dropped": [("261x512x256-s5", 2), ("785x768x2048-s8", 7), ("785x576x1024-s6", 11)],
    "acc_not_cleared": [("768x512x1024-s4", 1), ("785x448x768-s3", 7), ("8200x3072x256-s1", P.PRODUCTION)],
    "a_rows_prev": [("785x2304x256-s1", 7), ("768x512x1024-s4", 2)],
    "w_rows_prev": [("785x2304x256-s1", 5), ("785x448x768-s3", 1)],
    "ktile0_prev": [("785x768x2048-s8", 5), ("785x576x256-s1", 2), ("10989x2304x256-s1", 255)],
    "guard_cols_off": [("785x576x256-s1", 12), ("785x448x768-s3", 1), ("785x576x1024-s6", 5)],
    "guard_rows_off": [("261x512x256-s5", 3), ("785x2304x256-s1", 35), ("8200x3072x256-s1", P.PRODUCTION)],
    "last_slot_skipped": [("785x2304x256-s1", 7), ("10989x2304x256-s1", P.PRODUCTION)],
    "step_grid_minus_1": [("785x2304x256-s1", 7), ("768x512x1024-s4", 5), ("8200x3072x256-s1", 255)],
}
# ... and the defects the older shapes let through at every grid of theirs (no slot beyond the fourth, no guarded column tile)
PASSES_ON_OLD = ("late_slots_current_rows", "late_slots_dropped", "guard_cols_off")


def test_every_defect_is_named():
    assert set(REJECTED_BY) == set(P.DEFECTS)
    for pairs in REJECTED_BY.values():
        assert all(cid in BY_ID and grid in P.grids(BY_ID[cid]) for cid, grid in pairs), pairs


@pytest.mark.parametrize("defect", list(P.DEFECTS))
def test_planted_defect_is_rejected(defect):
    for cid, grid in REJECTED_BY[defect]:
        c = BY_ID[cid]
        v = P.verdict(c, P.emulate_walk(c, grid, defect))
        assert v is not None, f"{defect} ({P.DEFECTS[defect]}) passes on {cid} with {grid} workgroups"
        assert v[0] in ("decided", "sentinel"), f"{defect} on {cid}, {grid} workgroups: rejected by an undecided element only: {v[1]}"
        print(f"\n{defect} on {cid}, {grid} workgroups: {v[0]}: {v[1][:160]}")


@pytest.mark.parametrize("defect", PASSES_ON_OLD)
def test_the_older_shapes_let_it_through(defect):
    for c in P.OLD_CASES:
        for grid in P.OLD_GRIDS:
            v = P.verdict(c, P.emulate_walk(c, grid, defect))
            assert v is None, f"{defect} on {c.id}, {grid} workgroups: {v}"


@pytest.mark.parametrize("defect", [d for d in P.DEFECTS if d not in PASSES_ON_OLD])
def test_the_older_shapes_reject_the_rest(defect):
    """The other defects are within the older table's reach (the model agrees with what that test was written for)."""
    hits = [(c.id, grid) for c in P.OLD_CASES for grid in P.OLD_GRIDS[:3] if P.verdict(c, P.emulate_walk(c, grid, defect)) is not None]
    assert hits, defect
