"""Every (d, r) instance of the solve kernels against the oracle: the plain one-launch solve k_rtr_persist<D, R, SPLIT, MT,
false> in its four layouts on pose counts around the workgroup tile (A), the additive one k_rtr_persist<D, R, ., ., true> in
the three layouts additive_plan chooses by size (B), and the V-cycle kernels at 1, 2 and 4 lane groups per pose on every kind
of hierarchy (C).  The evaluation kernels have this matrix in tests/test_launch_geometry_gpu.py; the reduction primitives
for every (d+1) r in test_parity_gpu.py::test_in_kernel_reduction_primitives.

The cases are those of tests/solve_instance_cases.py; tests/test_solve_instance_cases_cpu.py checks on the oracle alone
that none of the oracle's decisions in them sits on a knife edge (solve_instance_cases.knife_edges), which is what makes
EQUAL iteration counts the right assertion; every oracle run of this file is checked the same way before it is compared.

Tolerances are the parity suite's: counts and statuses equal, iterate to 1e-7, cost to 1e-9 |f| + 1e-14 |X|^T |Q| |X|
(+ |X| . |G|), fInit and gradNormInit as tests/test_trust_region_branches_gpu.py, one V-cycle application to 1e-9.
"""
import ctypes as C

import numpy as np
import pytest

import solve_instance_cases as S
from conftest import device_tcg_mode, matrix_to_tiles, tiles_to_matrix, to_product_measurements
from solve_instance_cases import (ADDITIVE, ADDITIVE_LAYOUTS, DR, FOUR, GRAPH, KINDS, LAYOUTS, RUNS, RUNS_AP, THREE_LEVELS,
                                  TWO_TILES)
from test_launch_geometry_gpu import Guarded, Handle, guard_of, library_options, tile_poses
from test_parity_gpu import _hierarchy_check, relerr

pytestmark = pytest.mark.gpu


def cost_scale(op, X, G):
    Xa = np.abs(X).reshape(-1, X.shape[-1])
    scale = float((Xa * (abs(op.Qs) @ Xa)).sum())
    return scale + (float((np.abs(X) * np.abs(G)).sum()) if G is not None else 0.0)


def check_against_oracle(oracle, rg, Xg, op, ro, X0, Xo, G=None):
    """The device's result record and iterate against a verbose oracle run from the same start."""
    assert S.knife_edges(oracle, ro) == []  # (the input: see the module's docstring)
    accepted = [t["accept"] for t in ro.trace]
    assert rg.success, rg
    assert rg.rtr_iterations == ro.outer_iters == len(accepted), (rg, ro.outer_iters)
    assert rg.rtr_accepted == sum(accepted), (rg, accepted)
    assert rg.latest_step_accepted == bool(accepted[-1]), (rg, accepted)
    assert rg.tcg_iterations == ro.tcg_iters, (rg, ro.tcg_iters)
    assert rg.tCGStatus == oracle.TCG_NAMES[ro.tCGStatus], (rg, ro.tCGStatus)
    assert abs(rg.fInit - ro.fInit) <= 1e-14 * cost_scale(op, X0, G), (rg.fInit, ro.fInit)
    assert abs(rg.gradNormInit - ro.gradNormInit) <= 1e-10 * ro.gradNormInit, (rg.gradNormInit, ro.gradNormInit)
    assert relerr(Xg, Xo) < 1e-7, relerr(Xg, Xo)
    assert abs(rg.fOpt - ro.fOpt) <= 1e-9 * abs(ro.fOpt) + 1e-14 * cost_scale(op, Xo, G), (rg.fOpt, ro.fOpt)


# ---------------------------------------------------------------- A. plain one-launch solve
def persistent_info(h):
    v = [C.c_int(0) for _ in range(5)]
    h.L.check(h.lib.dpgo_problem_persistent_info(h.h, *[C.byref(x) for x in v]))
    out = dict(zip(("enabled", "workgroups", "last_members", "last_iterations"), (x.value for x in v[:4])))
    out["last_split"], out["last_tiles"] = v[4].value // 16, v[4].value % 16
    return out


def run_plain(oracle, lib, case, mt, entry, guard):
    """One plain case in the layout the library's switches force, through dpgo_optimize_device on an iterate between
    sentinel guards ("device") or through dpgo_optimize on host buffers ("host")."""
    import dpgo_amd
    from dpgo_amd.solver import ROPTResult
    d, r, n = case.d, case.r, case.n
    Qb, G, X0 = S.plain_problem(oracle, case)
    op, ro, _, Xo = S.plain_run(oracle, case, device_tcg_mode(n, d, r))
    h = Handle(lib, Qb, r, d)
    try:
        keep_G = None if G is None else np.ascontiguousarray(G)
        if keep_G is not None:
            h.L.check(lib.dpgo_problem_set_G(h.h, h.L.ptr(keep_G)))
        prm = dpgo_amd.ROptParameters(precond=case.precond, RTR_initial_radius=S.radius_of(case), time_bound_s=120.0,
                                      RTR_iterations=S.outer_of(case), RTR_tCG_iterations=S.inner_of(case))
        cp, cr = prm.to_c(), h.L.RoptResultC()
        if entry == "device":
            buf = Guarded(X0.size, guard, device=True, body=X0)
            h.L.check(lib.dpgo_optimize_device(h.h, C.byref(cp), buf.ptr(), C.byref(cr)))
        else:
            buf = Guarded(X0.size, guard, device=False)
            h.L.check(lib.dpgo_optimize(h.h, C.byref(cp), h.L.ptr(np.ascontiguousarray(X0)), buf.ptr(), C.byref(cr)))
        Xg = buf.result(X0.shape)  # (both guards intact, every entry written)
        rg = ROPTResult.from_c(cr)
        info = persistent_info(h)
        tiles = -(-n // tile_poses(d, case.split))
        # (a one-launch solve that timed out in the kernel falls back by itself: last_members is 0 then)
        assert info["enabled"] == 1 and info["last_members"] == info["workgroups"] == -(-tiles // mt) > 0, info
        assert (info["last_split"], info["last_tiles"]) == (case.split, mt), info
        assert rg.precond_used == case.precond, rg
        check_against_oracle(oracle, rg, Xg, op, ro, X0, Xo, G)
    finally:
        h.close()


@pytest.mark.parametrize("d,r", DR)
def test_plain_one_launch_solve_in_every_layout_on_ragged_sizes(oracle, d, r):
    """k_rtr_persist<D, R, SPLIT, MT, false> for (SPLIT, MT) = (4,1), (4,2), (1,1), (1,2), forced by DPGO_PERSIST_SPLIT /
    DPGO_PERSIST_MT on fresh handles: n = 2, P - 1, P, P + 1 (MT = 2: one workgroup whose second tile is empty), 2 P + 1 (an
    odd number of tiles), 17 P + 3 poses, P the split's tile (2-D: 21 or 5 poses per wave, idle lanes); block-Jacobi and
    none, without and with a linear term; through dpgo_optimize_device on an iterate between guards of at least one
    workgroup tile, and one case per layout through dpgo_optimize.  persistentInfo confirms the layout and the grid of
    every solve."""
    guard = guard_of(d, r)
    assert guard >= tile_poses(d, 1) * (d + 1) * r
    for split, mt in LAYOUTS:
        env = {"DPGO_PERSIST": "1", "DPGO_PERSIST_SPLIT": str(split), "DPGO_PERSIST_MT": str(mt)}
        with library_options(env) as lib:
            runs = [(c, "device") for c in S.plain_cases(d, r, split)] + [(S.host_entry_case(d, r, split), "host")]
            for case, entry in runs:
                try:
                    run_plain(oracle, lib, case, mt, entry, guard)
                except AssertionError as e:
                    raise AssertionError("%s, %d tiles per workgroup, %s entry: %s" % (case.name, mt, entry, e)) from e


# ---------------------------------------------------------------- B. additive one-launch solve
def device_problem(om, r):
    import dpgo_amd
    pg = dpgo_amd.PoseGraph(0, r, om.d)
    pg.setMeasurements(to_product_measurements(om))
    return dpgo_amd.QuadraticProblem(pg)


RUN_ADDITIVE = [c for c in ADDITIVE if c.dims]
RUN_ADDITIVE_IDS = ["%s-%s" % (c.name, c.layout.split(",")[0].replace(" ", "-")) for c in RUN_ADDITIVE]


@pytest.mark.parametrize("case", RUN_ADDITIVE, ids=RUN_ADDITIVE_IDS)
def test_additive_one_launch_solve_in_every_layout(oracle, case):
    """k_rtr_persist<D, R, 4, 1, true>, <D, R, 1, 1, true> and <D, R, 1, 2, true> at the (d, r) no other test runs them at
    (solve_instance_cases.ADDITIVE names the test of every other pair), on SE(d) lattices of the smallest sizes
    additive_plan puts into each layout; the plan is asserted first -- lane groups, tile, at most 256 aggregates, the
    hierarchy the rule restated on the oracle's aggregation gives -- so that a size that lands in another layout fails.
    Then as test_additive_preconditioner_matches_oracle: two calls, each from the oracle's iterate, against the oracle's
    precond = "amg_additive" on the same aggregates, counts and status equal, iterate to 1e-7, cost to 1e-9, one workgroup per aggregate, the hierarchy
    piece by piece.  Two tiles at (3, 6), where additive_lds_fits might have refused the plan: on the MI355X it fits, and
    test_two_tile_additive_matches_oracle[50x50x10-6] runs it with 230 aggregates."""
    import dpgo_amd
    d, r = case.d, case.r
    om, n, Q, X0 = S.lattice(oracle, d, case.dims, r, case.seed)
    prob = device_problem(om, r)
    lane_groups, tiles = ADDITIVE_LAYOUTS[case.layout]
    if case.layout == TWO_TILES:
        assert prob.additivePlan()["lane_groups"] == 0  # no one-tile plan holds the block
        assert prob.additiveTiles(2) == 2
    plan = prob.additivePlan()
    assert (plan["lane_groups"], plan["tile"]) == (lane_groups, tiles * tile_poses(d, lane_groups)), plan
    assert 0 < plan["aggregates"] <= 256 and plan["graph"], plan
    ks = plan["ks"]
    assert ks == S.additive_ks(oracle, Q, d, case.layout), plan
    op, rows = S.oracle_solve(oracle, Q, None, r, d, "amg_additive", X0, device_tcg_mode(n, d, r), calls=case.calls,
                              inner=case.inner, amg_k=ks)
    na = op.amg_setup()["nc"]
    assert na == plan["aggregates"]
    if case.layout == FOUR:  # a ragged last aggregate: some aggregate does not fill its tile
        assert n % plan["tile"] != 0 and na * plan["tile"] > n
    go = dpgo_amd.QuadraticOptimizer(prob, dpgo_amd.ROptParameters(precond="additive", RTR_tCG_iterations=case.inner,
                                                                    time_bound_s=120.0))
    for call, (ro, Xin, Xo) in enumerate(rows):  # (each call from the oracle's iterate: fInit is compared to round-off)
        Xg = matrix_to_tiles(go.optimize(tiles_to_matrix(Xin)), d)
        rg, info = go.getOptResult(), prob.persistentInfo()
        try:
            assert rg.precond_used == "additive", rg
            assert ro.gradNormInit >= 1e-2  # (an iterate that already meets the tolerance leaves before any launch)
            assert (info["last_members"], info["last_split"], info["last_tiles"]) == (na, lane_groups, tiles), (rg, info)
            check_against_oracle(oracle, rg, Xg, op, ro, Xin, Xo)
        except AssertionError as e:
            raise AssertionError("call %d: %s" % (call, e)) from e
    assert prob.multilevelInfo()["ks"] == ks
    _hierarchy_check(oracle, prob, op)


# ---------------------------------------------------------------- C. V-cycle
def apply_cycle(prob, X, V, guard):
    """One application of the multilevel preconditioner (dpgo_problem_precondition) into a guarded host buffer."""
    import dpgo_amd.lib as L
    o = Guarded(X.size, guard, device=False)
    L.check(prob._lib.dpgo_problem_precondition(prob.handle, L.PRECOND_MULTILEVEL, 0.1, L.ptr(np.ascontiguousarray(X)),
                                                L.ptr(np.ascontiguousarray(V)), o.ptr()))
    return o.result(X.shape)


@pytest.mark.parametrize("d,r", DR)
def test_vcycle_at_every_split_on_every_kind_of_hierarchy(oracle, d, r):
    """k_ml_presmooth, k_ml_restrict, k_ml_agg_sum, k_ml_coarse_prolong and the three post-smoothing kernels at DPGO_SPLIT =
    1, 2, 4 on graph aggregates (the default), on index runs (DPGO_ML_GRAPH=0: k_ml_post_ap) and on index runs with
    DPGO_ML_AP=0 (k_ml_post), and at 4 lane groups on an explicit three-level hierarchy (k_ml_post_mid): random graphs with
    a hub row, 17 P + 3 poses for the split's tile P and 257 poses (no run length divides it).  One application through a
    guarded host output against the oracle's cycle on the device's ks to 1e-9 (the oracle's BLAS on one thread), the
    hierarchy piece by piece once per kind."""
    from threadpoolctl import threadpool_limits
    guard = guard_of(d, r)
    checked = set()
    for case in S.cycle_cases(d, r):
        with library_options(dict(KINDS.get(case.kind, {}), DPGO_SPLIT=str(case.split))):
            om, Q, X, V = S.cycle_problem(oracle, case)
            prob = device_problem(om, r)
            try:
                assert "lane groups per pose %d;" % case.split in prob.describe()
                info = prob.setupMultilevel(S.three_level_ks(d) if case.kind == THREE_LEVELS else None)
                ks, levels, ap = info["ks"], len(info["sizes"]), prob.multilevelPath()["ap"]
                if case.kind == GRAPH:
                    assert ks[0] < 0 and levels == 2 and ap, info
                elif case.kind == RUNS_AP:
                    assert min(ks) > 0 and levels == 2 and ap, info
                elif case.kind == RUNS:
                    assert min(ks) > 0 and not ap, info
                else:
                    assert ks == S.three_level_ks(d) and levels == 3 and not ap, info
                assert any(case.n % k for k in ks if k > 0) or case.kind == GRAPH, info
                op = oracle.QuadraticProblem(Q, None, r, d, precond="amg", amg_k=ks)
                Zd = apply_cycle(prob, X, V, guard)
                with threadpool_limits(1):
                    Zo = op.precondition(X, V)
                assert relerr(Zd, Zo) < 1e-9, relerr(Zd, Zo)
                if case.kind not in checked:
                    checked.add(case.kind)
                    _hierarchy_check(oracle, prob, op)
            except AssertionError as e:
                raise AssertionError("%s: %s" % (case.name, e)) from e
            finally:
                del prob
    assert checked == set(KINDS) | {THREE_LEVELS}


@pytest.mark.parametrize("d,r", DR)
def test_multilevel_solve_at_every_rank(oracle, d, r):
    """A whole solve with the V-cycle (default hierarchy, default split, multi-launch) on an SE(d) lattice per (d, r) against
    the oracle on the device's hierarchy: counts and status equal, iterate to 1e-7, cost to 1e-9."""
    import dpgo_amd
    from threadpoolctl import threadpool_limits
    dims, seed = S.CYCLE_SOLVE[(d, r)]
    om, n, Q, X0 = S.lattice(oracle, d, dims, r, seed)
    with library_options({}):
        prob = device_problem(om, r)
        ks = prob.setupMultilevel()["ks"]
        assert ks == oracle.amg_default_ks(n, d + 1)  # (what tests/test_solve_instance_cases_cpu.py ran)
        with threadpool_limits(1):
            op, rows = S.oracle_solve(oracle, Q, None, r, d, "amg", X0, device_tcg_mode(n, d, r), amg_k=ks)
        ro, _, Xo = rows[0]
        go = dpgo_amd.QuadraticOptimizer(prob, dpgo_amd.ROptParameters(precond="multilevel", time_bound_s=120.0))
        Xg = matrix_to_tiles(go.optimize(tiles_to_matrix(X0)), d)
        rg = go.getOptResult()
        assert rg.precond_used == "multilevel" and prob.persistentInfo()["last_members"] == 0, rg
        check_against_oracle(oracle, rg, Xg, op, ro, X0, Xo)
        _hierarchy_check(oracle, prob, op)
        del go, prob
