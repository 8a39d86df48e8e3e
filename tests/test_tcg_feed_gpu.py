"""The host's feed of the tCG loop around the two-level V-cycle (solve.hip, rtr_outer_iteration): a step is enqueued only
after the device has published that it will run -- this run's generation for step 0, the go ticket of iteration s for step
s + 1 (progress word, kernels/common.h; published by the restriction's stop check, kernels/multilevel.h).

Nothing that is computed depends on the feed, so every case compares the default feed BITWISE -- iterate and result record
-- with polling mode (tcg_poll_interval = 1), which synchronises after every step and enqueues exactly what it needs, and
reads the feed counters (QuadraticProblem.feedCounters): steps enqueued - products <= 1 per run that was fed, and a run that
only discovers rtr_stop is fed nothing.  With DPGO_ML_EARLY_STOP=0 the feed stays two iterations ahead, as before: at most
two dead steps per run.

Blocks: smallGrid3D and tinyGrid3D (d = 3, r = 5), the 40 x 30 SE(2) lattice (r = 3) and sphere2500 from the trust-region
case table, all with the multilevel preconditioner forced and the one-launch solve switched off; every hierarchy is
asserted to have two levels with graph aggregates (the rule under test applies to two levels; graph aggregates add the
aggregate-sum launch to the cycle).  No oracle solve: polling mode is the reference.
"""
import numpy as np
import pytest

import trust_region_cases as C
from conftest import matrix_to_tiles, tiles_to_matrix, to_product_measurements
from test_launch_geometry_gpu import library_options
from trust_region_cases import Case

pytestmark = pytest.mark.gpu

SMALL = Case("smallGrid3D-5", ("data", "smallGrid3D"), 5, "multilevel", ("chordal",), 100.0, 0, (), ())
TINY = Case("tinyGrid3D-5", ("data", "tinyGrid3D"), 5, "multilevel", ("random", 3), 100.0, 0, (), ())
LATTICE = C.by_name("lattice-multilevel-1000-k0")  # 2-D: negative curvature, rejected; then the boundary, accepted
SPHERE = C.by_name("sphere2500-multilevel-k0")  # negative curvature twice, both rejected

_STARTS = {}


def start_of(oracle, case):
    if case.name not in _STARTS:
        assert case.k == 0  # (the window starts at the case's own start: no oracle trajectory)
        _STARTS[case.name] = C.window_start(oracle, case)
    return _STARTS[case.name]


def device_problem(oracle, case):
    import dpgo_amd
    p = C.build_problem(oracle, case)
    pg = dpgo_amd.PoseGraph(0, case.r, p["d"])
    pg.setMeasurements(to_product_measurements(p["om"]))
    prob = dpgo_amd.QuadraticProblem(pg)
    prob.setPersistent(False)
    info = prob.setupMultilevel()
    assert len(info["sizes"]) == 2 and info["ks"][0] < 0, info  # two levels, graph aggregates
    return prob


def parameters(radius, **kw):
    import dpgo_amd
    kw.setdefault("time_bound_s", 120.0)
    return dpgo_amd.ROptParameters(precond="multilevel", RTR_initial_radius=radius, **kw)


def record(rg):
    return (rg.success, rg.fInit, rg.gradNormInit, rg.fOpt, rg.gradNormOpt, rg.tCGStatus, rg.rtr_iterations, rg.rtr_accepted,
            rg.tcg_iterations, rg.spmm_count, rg.latest_step_accepted, rg.precond_used)


def solve(oracle, case, prob, **kw):
    """(iterate as tiles, result, feed counters) of one solve from the case's start."""
    import dpgo_amd
    X0, radius = start_of(oracle, case)
    opt = dpgo_amd.QuadraticOptimizer(prob, parameters(radius, **kw))
    Xg = matrix_to_tiles(opt.optimize(tiles_to_matrix(X0)), C.build_problem(oracle, case)["d"])
    rg = opt.getOptResult()
    assert rg.precond_used == "multilevel" and prob.persistentInfo()["last_members"] == 0, rg
    return Xg, rg, prob.feedCounters()


def fed_and_polled(oracle, case, prob=None, dead_per_run=None, **kw):
    """The same solve on the default feed and in polling mode: bitwise equal; the feed's counters within their bound
    (dead_per_run = None: one dead step per FED run; a number: that many per run started, the rule of the other paths)."""
    prob = prob or device_problem(oracle, case)
    Xf, rf, cf = solve(oracle, case, prob, **kw)
    Xp, rp, cp = solve(oracle, case, prob, tcg_poll_interval=1, **kw)
    what = (case.name, kw, rf, cf, rp, cp)
    assert np.array_equal(Xf.view(np.uint64), Xp.view(np.uint64)), what
    assert record(rf) == record(rp), what
    assert cf["products"] == rf.tcg_iterations == cp["products"], what
    # (polling mode reads rtr_stop back and starts no run behind it; the feed learns it from that run's opening update)
    assert cp["runs"] <= cf["runs"] <= cp["runs"] + 1 and 0 <= cf["runs_fed"] <= cf["runs"], what
    assert cf["dead_iterations"] == cf["steps"] - cf["products"] >= 0, what
    if dead_per_run is None:
        assert cf["dead_iterations"] <= cf["runs_fed"], what
        assert cf["runs_fed"] == cp["runs_fed"], what  # (a run is fed exactly when it has a first product to compute)
    else:
        assert cf["dead_iterations"] <= dead_per_run * cf["runs"], what
    return rf, cf


def test_residual_test_ends_the_runs(oracle):
    """smallGrid3D from the chordal start, reference defaults: the runs end on tCG's residual test (the restriction's stop
    check, or the Hessian step's prologue), and the solve on the gradient-norm tolerance or after three outer iterations."""
    rg, cnt = fed_and_polled(oracle, SMALL)
    assert rg.tCGStatus in (C.LCON, C.SCON) and rg.tcg_iterations > rg.rtr_iterations, rg
    assert cnt["runs_fed"] == rg.rtr_iterations, (rg, cnt)


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_iteration_cap_binds(oracle, cap):
    """RTR_tCG_iterations = 1, 2, 3: every run reaches the cap; the closing Hessian-step launch finalises it."""
    rg, cnt = fed_and_polled(oracle, SMALL, RTR_tCG_iterations=cap, gradnorm_tol=1e-12)
    assert rg.tCGStatus == C.MAXIT and rg.rtr_iterations == 3 and rg.tcg_iterations == 3 * cap, rg
    assert cnt["steps"] == 3 * cap and cnt["runs"] == cnt["runs_fed"] == 3, cnt


def test_no_inner_iterations(oracle):
    """RTR_tCG_iterations = 0: nothing is fed, every run is its opening launches and the finalising one."""
    rg, cnt = fed_and_polled(oracle, SMALL, RTR_tCG_iterations=0, gradnorm_tol=1e-12)
    assert rg.tcg_iterations == 0 and cnt["steps"] == 0 and cnt["runs_fed"] == 0 and cnt["runs"] == rg.rtr_iterations, (rg, cnt)


def test_start_meets_the_tolerance(oracle):
    """A tolerance above the start's gradient norm: the first run's opening update publishes rtr_stop -- the solve has
    started one run, fed it nothing and returns the input."""
    X0, _ = start_of(oracle, SMALL)
    prob = device_problem(oracle, SMALL)
    rg, cnt = fed_and_polled(oracle, SMALL, prob=prob, gradnorm_tol=1e9)
    assert rg.rtr_iterations == 0 and rg.tcg_iterations == 0 and rg.fOpt == rg.fInit, rg
    assert (cnt["runs"], cnt["runs_fed"], cnt["steps"]) == (1, 0, 0), cnt
    Xg, _, _ = solve(oracle, SMALL, prob, gradnorm_tol=1e9)
    assert np.array_equal(Xg.view(np.uint64), np.ascontiguousarray(X0).view(np.uint64))


@pytest.mark.parametrize("after", [1, 2])
def test_stop_test_met_after_an_outer_iteration(oracle, after):
    """The gradient-norm tolerance just above the norm after the first / the second outer iteration: k_rtr_update raises
    rtr_stop on the device, the next run discovers it in its opening update and is fed nothing."""
    prob = device_problem(oracle, SMALL)
    norms = []
    for its in (1, 2):  # (RTR_iterations = 1 is the shrink loop: its first try is the first outer iteration)
        _, r, _ = solve(oracle, SMALL, prob, RTR_iterations=its, gradnorm_tol=1e-12, tcg_poll_interval=1)
        assert r.rtr_accepted == its and r.rtr_iterations == its, r
        norms.append(r.gradNormOpt)
    assert norms[0] > 1.001 * norms[1] > 0.0, norms
    rg, cnt = fed_and_polled(oracle, SMALL, prob=prob, gradnorm_tol=norms[after - 1] * (1.0 + 1e-6))
    assert rg.rtr_iterations == after, (rg, norms)
    assert (cnt["runs"], cnt["runs_fed"]) == (after + 1, after), cnt


@pytest.mark.parametrize("case", [LATTICE, SPHERE, TINY], ids=lambda c: c.name)
def test_boundary_negative_curvature_and_rejected_steps(oracle, case):
    """Windows of the trust-region case table on the V-cycle (tests/test_trust_region_branches_gpu.py holds them against
    the oracle): the 2-D lattice leaves tCG through negative curvature, is rejected, runs again and ends on the boundary;
    sphere2500 from a random point is rejected twice; tinyGrid3D from a random point with the reference defaults."""
    kw = dict(RTR_iterations=len(case.expect), RTR_tCG_iterations=case.tcg_iterations) if case.expect else {}
    rg, cnt = fed_and_polled(oracle, case, **kw)
    if case.expect:
        accepted = [e[2] == C.ACC for e in case.expect]
        assert (rg.rtr_iterations, rg.rtr_accepted, rg.tCGStatus, rg.latest_step_accepted) == (
            len(accepted), sum(accepted), case.expect[-1][0], accepted[-1]), rg
        assert not all(accepted) and cnt["runs_fed"] == len(accepted), (rg, cnt)


def test_time_bound_between_outer_iterations(oracle):
    """A time bound that has passed when the first outer iteration has been enqueued: the solve returns that iteration's
    record, as in polling mode -- one run, no second one started."""
    rg, cnt = fed_and_polled(oracle, SMALL, time_bound_s=1e-9, gradnorm_tol=1e-12)
    assert rg.rtr_iterations == 1 and rg.tcg_iterations > 0, rg
    assert (cnt["runs"], cnt["runs_fed"]) == (1, 1), cnt


@pytest.mark.parametrize("case", [SMALL, LATTICE], ids=lambda c: c.name)
def test_without_the_early_stop_the_feed_stays_two_ahead(oracle, case):
    """DPGO_ML_EARLY_STOP=0: no ticket is published, the feed keeps its rule -- at most two dead steps per run."""
    with library_options({"DPGO_ML_EARLY_STOP": "0"}):
        kw = dict(RTR_iterations=len(case.expect), RTR_tCG_iterations=case.tcg_iterations) if case.expect else {}
        prob = device_problem(oracle, case)
        fed_and_polled(oracle, case, prob=prob, dead_per_run=2, **kw)
        del prob


@pytest.mark.parametrize("count", [2, 3])
def test_handles_side_by_side(oracle, count):
    """optimize_device_many with 2 and 3 handles (one feeding thread each, every one waiting on its own progress word):
    every handle's iterate and record are those of a handle solved alone with the same parameters."""
    import torch
    import dpgo_amd
    from dpgo_amd.solver import optimize_device_many
    cases = [SMALL, LATTICE, SMALL][:count]
    prm = parameters(100.0)  # (one parameter record for all handles)

    def on_device(case):
        return torch.from_numpy(np.ascontiguousarray(start_of(oracle, case)[0]).reshape(-1).copy()).cuda()

    alone = {}
    for case in set(cases):
        prob, x = device_problem(oracle, case), on_device(case)
        r = dpgo_amd.QuadraticOptimizer(prob, prm).optimizeDevice(x)
        torch.cuda.synchronize()
        alone[case.name] = (x.cpu().numpy().view(np.uint64).copy(), record(r))
        del prob
    probs = [device_problem(oracle, case) for case in cases]
    xs = [on_device(case) for case in cases]
    results = optimize_device_many([dpgo_amd.QuadraticOptimizer(p, prm) for p in probs], xs)
    torch.cuda.synchronize()
    for k, (case, prob, x, rg) in enumerate(zip(cases, probs, xs, results)):
        cnt = prob.feedCounters()
        assert prob.persistentInfo()["last_members"] == 0
        assert np.array_equal(x.cpu().numpy().view(np.uint64), alone[case.name][0]), (k, case.name)
        assert record(rg) == alone[case.name][1], (k, case.name, rg, alone[case.name][1])
        assert cnt["products"] == rg.tcg_iterations > 0 and 0 <= cnt["dead_iterations"] <= cnt["runs_fed"], (k, cnt)
