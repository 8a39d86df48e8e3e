"""The case table of tests/solve_instance_cases.py is complete, and its cases are fit for an exact comparison of
iteration counts -- on the oracle alone (no GPU).

Completeness: every (d, r) x (SPLIT, MT) of the plain one-launch solve with every pose count, preconditioner and the
linear term; every (d, r) x layout of the additive one; every (d, r) x DPGO_SPLIT x hierarchy kind of the V-cycle.  Fitness
(solve_instance_cases.knife_edges): no rho within 0.01 of 0.1 / 0.25 / 0.75, no tCG residual within 10 % of the stopping
threshold at the step that stops or the one before it, no step within 10 % of the radius in front of a boundary exit, no
other decision within 1 %; and the run is well conditioned (solve_instance_cases.instabilities): from a start 1e-15 away
the oracle takes the same decisions and ends within 1e-10 of its iterate.  These are conditions on the INPUTS: a case that misses one gets another seed, start or radius
(SEEDS), never a looser assertion on the device side.  The additive cases on one and two whole tiles (4 400 - 21 600
poses) are too slow for this file; tests/test_solve_instances_gpu.py applies the same check to its own oracle runs.
"""
import os

import numpy as np
import pytest

import solve_instance_cases as S
from solve_instance_cases import (ADDITIVE, ADDITIVE_FOUR, ADDITIVE_LAYOUTS, ADDITIVE_ONE_TILE, ADDITIVE_TWO_TILES, DR, FOUR,
                                  KINDS, LAYOUTS, ONE_TILE, SPLITS, THREE_LEVELS, TWO_TILES)


def test_tables_are_complete():
    # A: both lane-group counts, six pose counts around each one's tile, two preconditioners, without and with G
    for d, r in DR:
        for split, mt in LAYOUTS:
            cases = S.plain_cases(d, r, split)
            P = S.tile_poses(d, split)
            assert {c.n for c in cases} == {2, P - 1, P, P + 1, 2 * P + 1, 17 * P + 3}
            assert {(c.n, c.precond, c.linear) for c in cases} == {(n, pc, g) for n in S.pose_counts(d, split)
                                                                   for pc in ("jacobi", "none") for g in (False, True)}
            assert S.host_entry_case(d, r, split) in cases
    assert sorted(LAYOUTS) == [(1, 1), (1, 2), (4, 1), (4, 2)]
    assert set(S.SEEDS) <= {c.key for d, r in DR for c in S.plain_cases(d, r)}  # (no entry for a case that is gone)
    # B: 24 (d, r, layout) cases, each run here or named as run by an existing test
    assert [(c.d, c.r) for c in ADDITIVE_FOUR] == DR and all(c.layout == FOUR for c in ADDITIVE_FOUR)
    assert [(c.d, c.r) for c in ADDITIVE_ONE_TILE] == DR and all(c.layout == ONE_TILE for c in ADDITIVE_ONE_TILE)
    assert [(c.d, c.r) for c in ADDITIVE_TWO_TILES] == DR and all(c.layout == TWO_TILES for c in ADDITIVE_TWO_TILES)
    assert len(ADDITIVE) == 24 and set(ADDITIVE_LAYOUTS) == {FOUR, ONE_TILE, TWO_TILES}
    for c in ADDITIVE:
        assert bool(c.dims) != bool(c.covered), c
        if c.covered:  # the named test exists and has that parameter set
            module, rest = c.covered.split("::")
            name, param = rest.rstrip("]").split("[")
            text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), module)).read()
            assert "def %s(" % name in text, c.covered
            workload, rank = param.rsplit("-", 1)
            assert int(rank) == c.r and ('"%s", %d' % (workload, c.r) in text or '"%s"' % workload in text), c.covered
    # C: every (d, r) x split x kind, three levels at 4 lane groups, a pose count no run length divides
    for d, r in DR:
        cases = S.cycle_cases(d, r)
        assert {(c.split, c.kind) for c in cases} >= {(s, k) for s in SPLITS for k in KINDS} | {(4, THREE_LEVELS)}
        assert all(c.n == 17 * S.tile_poses(d, c.split) + 3 or c.n == 257 for c in cases)
        assert any(c.n % k for c in cases for k in (2, 4, 5, 8, 16, 20))
        assert all(S.tile_poses(d, 4) % k == 0 for k in S.three_level_ks(d))
    assert sorted(S.CYCLE_SOLVE) == DR


@pytest.mark.parametrize("d,r", DR)
def test_plain_cases_are_off_every_knife_edge(oracle, d, r):
    for case in S.plain_cases(d, r):
        op, res, X0, Xo = S.plain_run(oracle, case)
        assert S.outer_of(case) >= 2  # (RTR_iterations = 1 is the multi-launch shrink loop)
        assert res.outer_iters == len(res.trace) >= 1, case.name
        assert S.knife_edges(oracle, res) == [], case.name
        assert S.plain_instabilities(oracle, case) == [], case.name
        assert res.gradNormInit >= 1e-2, case.name  # the solve launches


def _aggregates(oracle, Q, S_):
    return len(oracle.amg_graph_aggregates(Q, S_)[1]) - 1


@pytest.mark.parametrize("case", [c for c in ADDITIVE if c.dims], ids=lambda c: c.name + "-" + c.layout.split(",")[0])
def test_additive_sizes_land_in_their_layout(oracle, case):
    """additive_plan's rules (csrc/multilevel.hip) restated with the oracle's aggregation: growth to one 4-lane-group tile
    leaves at most 256 aggregates for the `4 lane groups` cases and more for the others; one tile of one pose per (d+1)
    lanes holds the one-tile cases (n <= 256 tiles, just above the four-group limit) and cannot hold the two-tile ones."""
    om, n, Q, X0 = S.lattice(oracle, case.d, case.dims, case.r, case.seed)
    P4, P1 = S.tile_poses(case.d, 4), S.tile_poses(case.d, 1)
    na4 = _aggregates(oracle, Q, P4) if n <= 256 * P4 else None
    if case.layout == FOUR:
        assert 100 <= n <= 999 and n % P4 != 0 and na4 is not None and na4 <= 256
    elif case.layout == ONE_TILE:
        assert (na4 is None or na4 > 256) and n <= 256 * P1
        assert (4200 <= n <= 4500) if case.d == 3 else (5200 <= n <= 5600)
    else:
        assert 256 * P1 < n <= 256 * P1 + 700


@pytest.mark.parametrize("case", [c for c in ADDITIVE_FOUR if c.dims], ids=lambda c: c.name)
def test_small_additive_cases_are_off_every_knife_edge(oracle, case):
    om, n, Q, X0 = S.lattice(oracle, case.d, case.dims, case.r, case.seed)
    op, rows = S.oracle_solve(oracle, Q, None, case.r, case.d, "amg_additive", X0, calls=case.calls,
                              inner=case.inner, amg_k=S.four_group_ks(case.d))
    assert op.amg_setup()["nc"] <= 256
    for res, Xin, Xout in rows:
        assert S.knife_edges(oracle, res) == [], case.name
    assert S.instabilities(oracle, op, rows, lambda X, rec: S.oracle_solve(
        oracle, Q, None, case.r, case.d, "amg_additive", X, rec, calls=case.calls, inner=case.inner,
        amg_k=S.four_group_ks(case.d))[1]) == []


@pytest.mark.parametrize("d,r", DR)
def test_vcycle_solve_cases_are_off_every_knife_edge(oracle, d, r):
    from threadpoolctl import threadpool_limits
    dims, seed = S.CYCLE_SOLVE[(d, r)]
    om, n, Q, X0 = S.lattice(oracle, d, dims, r, seed)
    runs = []
    for limit in (1, None):  # (the dense level goes through BLAS: the run must not depend on how its threads split it)
        with threadpool_limits(limit):
            op, rows = S.oracle_solve(oracle, Q, None, r, d, "amg", X0, amg_k=oracle.amg_default_ks(n, d + 1))
        runs.append(rows[0][0])
    assert S.knife_edges(oracle, runs[0]) == []
    assert S.instabilities(oracle, op, rows, lambda X, rec: S.oracle_solve(oracle, Q, None, r, d, "amg", X, rec,
                                                                          amg_k=oracle.amg_default_ks(n, d + 1))[1]) == []
    assert (runs[0].tcg_iters, runs[0].outer_iters) == (runs[1].tcg_iters, runs[1].outer_iters)
    assert [t["status"] for t in runs[0].trace] == [t["status"] for t in runs[1].trace]
    for c in S.cycle_cases(d, r):  # and the inputs of the single applications exist at every size
        assert np.isfinite(S.cycle_problem(oracle, c)[3]).all()
