"""The additive one-launch solve on TWO-tile aggregates (dpgo_problem_additive_tiles = 2, opt-in): blocks of 16 000 -
~28 000 poses in 3-D, which no one-tile plan holds, get graph aggregates of at most 128 poses on the two 64-pose tiles of a
workgroup (k_rtr_persist<3, R, 1, 2, true>), checked against the oracle's restatement of the operator
(precond = "amg_additive", same aggregates)."""
import numpy as np
import pytest

from conftest import matrix_to_tiles, tiles_to_matrix, to_product_measurements, device_tcg_mode
from test_parity_gpu import _additive_growth_sizes, _grid2d_measurements, _hierarchy_check, relerr

pytestmark = pytest.mark.gpu

# 18 000 and 25 000 poses (the N = 2 rank share of the 100k grid), and 28 800: the schedule's growth sizes stop at 128
# poses, so n <= 230 x 128 = 29 440
GRIDS = ["30x30x20", "50x50x10", "40x40x18"]


def _grid_problem(oracle, dims, r=5):
    """3-D synthetic grid "NXxNYxNZ" (perturbed truth), or "grid2d:NXxNY": the random-measurement SE(2) lattice (chordal)."""
    import dpgo_amd
    if dims.startswith("grid2d:"):
        om, n = _grid2d_measurements(oracle, *[int(v) for v in dims[7:].split("x")], seed=4)
        X0 = oracle.lift(oracle.chordal_initialization(om, n), r)
    else:
        om, n, Ttrue = oracle.synthetic_grid(*[int(v) for v in dims.split("x")], seed=0)
        X0 = oracle.lift(oracle.perturbed_truth(Ttrue, seed=2), r)
    pg = dpgo_amd.PoseGraph(0, r, om.d)
    pg.setMeasurements(to_product_measurements(om))
    return om, n, X0, dpgo_amd.QuadraticProblem(pg)


@pytest.mark.parametrize("dims", GRIDS)
def test_two_tile_plan(oracle, dims):
    """additivePlan() with the opt-in: one pose per (d+1) lanes, 128-slot aggregates, at most 256 of them, grown from the
    smallest size of the schedule that fits and merged up to min(128, S + S / 2); without the opt-in (before and after)
    the same handle has no plan."""
    om, n, X0, prob = _grid_problem(oracle, dims)
    assert prob.additiveTiles() == 1
    assert prob.additivePlan()["lane_groups"] == 0
    assert prob.additiveTiles(2) == 2 and prob.additiveTiles() == 2
    plan = prob.additivePlan()
    assert plan["lane_groups"] == 1 and plan["tile"] == 128 and plan["graph"], plan
    S = plan["growth"]
    assert -plan["ks"][1] == min(128, S + S // 2) and plan["ks"][0] == -S
    Q = oracle.construct_Q(n, om.d, om)
    lab, ptr, mem, _, _ = oracle.amg_graph_aggregates(Q, S)
    got = oracle.amg_merge_small_aggregates(Q, S, lab, ptr, mem, min(128, S + S // 2))
    assert len(got[1]) - 1 == plan["aggregates"] <= 256
    for s_ in [s_ for s_ in _additive_growth_sizes(n, 128) if s_ < S]:  # every earlier size leaves more than 256
        lab, ptr, mem, _, _ = oracle.amg_graph_aggregates(Q, s_)
        assert len(oracle.amg_merge_small_aggregates(Q, s_, lab, ptr, mem, min(128, s_ + s_ // 2))[1]) - 1 > 256
    assert prob.additiveTiles(1) == 1
    assert prob.additivePlan()["lane_groups"] == 0


@pytest.mark.parametrize("dims,r", [(g, 5) for g in GRIDS] + [("50x50x10", 6), ("grid2d:160x160", 5)])
def test_two_tile_additive_matches_oracle(oracle, dims, r):
    """precond = "additive" on a two-tile plan: three calls against the oracle at matched settings -- same RTR / tCG counts
    and status, iterate to 1e-7, cost to 1e-9 --, each call one launch on one workgroup per aggregate with two tiles, and
    the device's hierarchy is the oracle's.  Also r = 6 (the largest static LDS of the two-tile instances, with 256
    aggregates' coarse rows still within the CU) and the 2-D layout (168-slot aggregates, odd (d+1) r: column-wise
    publication) on a 25 600-pose SE(2) lattice, there six calls each from the ORACLE's previous iterate (every call of
    that far-from-optimal lattice ends on the trust-region boundary)."""
    import dpgo_amd
    om, n, X0, prob = _grid_problem(oracle, dims, r)
    d = om.d
    prob.additiveTiles(2)
    plan = prob.additivePlan()
    assert plan["lane_groups"] == 1 and plan["tile"] == 2 * (64 // (d + 1)) * 4, plan
    ks = plan["ks"]
    op = oracle.QuadraticProblem(oracle.construct_Q(n, d, om), None, r, d, precond="amg_additive", amg_k=ks)
    na = op.amg_setup()["nc"]
    assert na == plan["aggregates"] <= 256
    oo = oracle.QuadraticOptimizer(op, oracle.ROptParameters(), hess_recurrence=True)
    go = dpgo_amd.QuadraticOptimizer(prob, dpgo_amd.ROptParameters(precond="additive"))
    Xo, Xg = X0, X0
    resync = d == 2
    for call in range(6 if resync else 3):
        if resync:
            Xg = Xo
        Xo = oo.optimize(Xo)
        Xg = matrix_to_tiles(go.optimize(tiles_to_matrix(Xg)), d)
        rg = go.getOptResult()
        info = prob.persistentInfo()
        assert rg.precond_used == "additive"
        if rg.gradNormInit >= 1e-2:
            assert (info["last_members"], info["last_split"], info["last_tiles"]) == (na, 1, 2), (rg, info)
        assert (rg.tcg_iterations, rg.rtr_iterations, rg.tCGStatus) == (oo.result.tcg_iters, oo.result.outer_iters,
                                                                         oracle.TCG_NAMES[oo.result.tCGStatus]), call
        assert relerr(Xg, Xo) < 1e-7
        Xa = np.abs(Xo).reshape(n * (d + 1), r)
        scale = float((Xa * (abs(op.Qs) @ Xa)).sum())
        assert abs(rg.fOpt - oo.result.fOpt) <= 1e-9 * abs(oo.result.fOpt) + 1e-14 * scale
    assert prob.multilevelInfo()["ks"] == ks
    _hierarchy_check(oracle, prob, op)


def test_two_tile_additive_falls_back_to_the_vcycle_on_the_same_hierarchy(oracle):
    """With the one-launch solve switched off, "additive" on a 25 000-pose two-tile plan runs the multi-launch V-cycle on
    the same 128-pose hierarchy (restriction run table and aggregate sums over 128-member aggregates) and reaches the
    optimum the one-launch solve reaches."""
    import dpgo_amd
    om, n, X0, prob = _grid_problem(oracle, "50x50x10")
    d = om.d
    prob.additiveTiles(2)
    ks = prob.additivePlan()["ks"]
    na = prob.additivePlan()["aggregates"]
    go = dpgo_amd.QuadraticOptimizer(prob, dpgo_amd.ROptParameters(precond="additive"))
    X = X0
    for call in range(10):
        X = matrix_to_tiles(go.optimize(tiles_to_matrix(X)), d)
        if call == 0:  # the reference optimum is the one-launch solve's: its first call ran on the two-tile layout
            info = prob.persistentInfo()
            assert (info["last_members"], info["last_tiles"]) == (na, 2), info
        if go.getOptResult().gradNormOpt < 1e-2:
            break
    f_add = go.getOptResult().fOpt
    assert go.getOptResult().gradNormOpt < 1e-2
    prob.setPersistent(False)
    go2 = dpgo_amd.QuadraticOptimizer(prob, dpgo_amd.ROptParameters(precond="additive"))
    X = X0
    for _ in range(10):
        X = matrix_to_tiles(go2.optimize(tiles_to_matrix(X)), d)
        assert prob.persistentInfo()["last_members"] == 0
        if go2.getOptResult().gradNormOpt < 1e-2:
            break
    assert go2.getOptResult().gradNormOpt < 1e-2
    assert abs(go2.getOptResult().fOpt - f_add) <= 1e-7 * abs(f_add)
    assert prob.multilevelInfo()["ks"] == ks


def test_two_tile_additive_rbcd_of_two_coupled_blocks_matches_oracle(oracle):
    """grid:50x50x20 cut into 2 agents of 25 000 poses (the N = 2 rank share of the 100k workload): coloured RBCD sweeps
    with precond = "additive" on the two-tile plans, against the oracle driver at matched settings."""
    import dpgo_amd
    from dpgo_amd.agent import DeviceAgent, ExchangePlan, RBCDCluster, build_pose_graphs
    r, robots, sweeps = 5, 2, 2
    om, n, Ttrue = oracle.synthetic_grid(50, 50, 20, seed=0)
    X0 = oracle.lift(oracle.perturbed_truth(Ttrue, seed=2), r)
    d = om.d
    ranges, graphs = build_pose_graphs(to_product_measurements(om), n, robots, r)
    plan = ExchangePlan(graphs)
    agents = {a: DeviceAgent(graphs, plan, a, X0[ranges[a][0]:ranges[a][1]], dpgo_amd.ROptParameters(precond="additive"))
              for a in range(robots)}
    for a in range(robots):
        agents[a].problem.additiveTiles(2)
    plans = {a: agents[a].problem.additivePlan() for a in range(robots)}
    assert all(pl["lane_groups"] == 1 and pl["tile"] == 128 and pl["graph"] for pl in plans.values()), plans
    amg_k = {a: plans[a]["ks"] for a in range(robots)}
    Xref, costs, gns = oracle.rbcd_coloured(om, n, robots, r, X0, sweeps, hess_recurrence=device_tcg_mode(n // robots, d, r),
                                            precond="amg_additive", amg_k=amg_k)
    cluster = RBCDCluster(plan, agents)
    for k in range(sweeps):
        cluster.sweep()
        f, g = cluster.central_cost_and_gradnorm()
        assert abs(2 * f - costs[k]) <= 1e-9 * abs(costs[k])
        assert abs(g - gns[k]) <= 1e-6 * gns[k]
    X = np.concatenate([agents[a].X.cpu().numpy() for a in range(robots)], axis=0)
    assert relerr(X, Xref) < 1e-7
    for a in range(robots):
        res, info = agents[a].optimizer.getOptResult(), agents[a].problem.persistentInfo()
        assert res.precond_used == "additive", (a, res)
        assert (info["last_members"], info["last_tiles"]) == (plans[a]["aggregates"], 2), (a, res, info)
        assert agents[a].problem.multilevelInfo()["ks"] == plans[a]["ks"]


def test_auto_moves_coupled_two_tile_blocks_to_additive(oracle):
    """precond = "auto" with the opt-in on the 2 x 25 000 cut of grid:50x50x20: the coupled blocks start on block-Jacobi
    and, once block-Jacobi has cost one hierarchy set-up, move to the two-tile additive one-launch solve (the rule charges
    it its own unit); without the opt-in the same blocks never run additive."""
    import dpgo_amd
    from dpgo_amd.agent import DeviceAgent, ExchangePlan, RBCDCluster, build_pose_graphs
    r, robots = 5, 2
    om, n, Ttrue = oracle.synthetic_grid(50, 50, 20, seed=0)
    X0 = oracle.lift(oracle.perturbed_truth(Ttrue, seed=2), r)
    ranges, graphs = build_pose_graphs(to_product_measurements(om), n, robots, r)
    used = {}
    for tiles in (1, 2):
        plan = ExchangePlan(graphs)
        agents = {a: DeviceAgent(graphs, plan, a, X0[ranges[a][0]:ranges[a][1]], dpgo_amd.ROptParameters(precond="auto"))
                  for a in range(robots)}
        for a in range(robots):
            assert agents[a].problem.additiveTiles(tiles) == tiles
        cluster = RBCDCluster(plan, agents)
        f_first = None
        seen = set()
        for _ in range(10):
            cluster.sweep()
            f, _g = cluster.central_cost_and_gradnorm()
            f_first = f if f_first is None else f_first
            for a in range(robots):
                res, info = agents[a].optimizer.getOptResult(), agents[a].problem.persistentInfo()
                seen.add(res.precond_used)
                if res.precond_used == "additive":
                    assert (info["last_members"], info["last_tiles"]) == (agents[a].problem.additivePlan()["aggregates"], 2)
                    assert agents[a].problem.autoInfo()["state"] in ("additive", "trial"), agents[a].problem.autoInfo()
        assert f < f_first
        used[tiles] = seen
    assert "additive" not in used[1], used
    assert "additive" in used[2] and "jacobi" in used[2], used
