"""Rejected steps, the three rho bands, the radius clipped at Delta_max and tCG's negative-curvature exit on every solve
path of the device, against the oracle at matched settings.

The cases are the windows of tests/trust_region_cases.py (tests/test_trust_region_cases_cpu.py checks on the oracle alone
that each takes the branches it records, with every rho at least 0.01 from a threshold, and that the table holds every
(path, branch) pair).  A window is 2 - 4 outer iterations from an iterate of a long oracle trajectory with the radius the
trajectory had there, run freshly on both sides; the first iteration takes the branch, the following ones show that the
state after it -- the OLD point, gradient, S, dinv and radius / 4 after a rejection -- was right.

Asserted per window with the parity suite's tolerances: rtr_iterations, rtr_accepted, latest_step_accepted, tcg_iterations
and tCGStatus equal to the oracle's; iterate to 1e-7; cost to 1e-9 |f| + 1e-14 |X|^T |Q| |X| (+ |X| . |G| with a linear
term); fInit, gradNormInit as in test_optimize_matches_oracle_at_matched_settings.

accept_tiny_decrease = False runs one rejecting window per path on both sides.  A window in which the clause ITSELF
decides (rho <= 0.1, f2 < f1, relative decrease below sqrt(eps)) is not in the table: the oracle was searched for one
(random and chordal starts on the random graphs, sphere2500, kitti_00 and torus3D, block-Jacobi and none, trust radii
1e-3 ... 1e-10, three iterations each): with a radius that small the quadratic model is exact to round-off and rho stays
within 4 % of 1 down to relative decreases of 1e-15; the clause decided in none of 336 iterations.  Nothing is asserted
about it here rather than asserting on the round-off of f.
"""
import contextlib

import numpy as np
import pytest

import trust_region_cases as C
from conftest import matrix_to_tiles, tiles_to_matrix, to_product_measurements, device_tcg_mode
from test_launch_geometry_gpu import Guarded, guard_of, library_options
from test_parity_gpu import relerr
from trust_region_cases import (ADD1, ADD2, BEGIN_END, CASES, DEVICE, ENTRIES, LINEAR, MANY, MULTI, ONE, POLL, REJ, SYM, SYM_HOST,
                                VCYCLE)

pytestmark = pytest.mark.gpu

_ORACLE_RUNS = {}


def oracle_window(oracle, case, tiny=None):
    """(X0, radius, optimizer, Xopt) of the oracle on the case's window, cached (several paths run the same window)."""
    key = (case.name, case.tiny if tiny is None else tiny)
    if key not in _ORACLE_RUNS:
        p = C.build_problem(oracle, case)
        one_thread = contextlib.nullcontext()
        if case.precond == "multilevel":  # (the oracle's BLAS on one thread, as test_multilevel_on_random_graphs_...)
            from threadpoolctl import threadpool_limits
            one_thread = threadpool_limits(1)
        with one_thread:
            _ORACLE_RUNS[key] = C.run_window(oracle, case, tiny=tiny, hess_recurrence=device_tcg_mode(p["n"], p["d"], case.r))
    return _ORACLE_RUNS[key]


def device_problem(oracle, case):
    import dpgo_amd
    import dpgo_amd.lib as L
    p = C.build_problem(oracle, case)
    pg = dpgo_amd.PoseGraph(0, case.r, p["d"])
    pg.setMeasurements(to_product_measurements(p["om"]))
    assert pg.n() == p["n"]
    prob = dpgo_amd.QuadraticProblem(pg, host_linear_term=p["G"] is None)
    if p["G"] is not None:  # the multi-agent cost: G through the C ABI, as tiles [n, d+1, r]
        prob._keep_G = np.ascontiguousarray(p["G"])
        L.check(prob._lib.dpgo_problem_set_G(prob.handle, L.ptr(prob._keep_G)))
    return prob


def device_parameters(oracle, case, radius, tiny=None, **extra):
    import dpgo_amd
    return dpgo_amd.ROptParameters(precond=case.precond, accept_tiny_decrease=case.tiny if tiny is None else tiny,
                                   time_bound_s=120.0, **C.window_parameters(oracle, case, radius), **extra)


def check_result(oracle, case, rg, Xg, run, what):
    """The device's result record and iterate against the oracle's run of the same window."""
    X0, radius, oo, Xo = run
    ro, p = oo.result, C.build_problem(oracle, case)
    accepted = [t["accept"] for t in ro.trace]
    assert C.observed(oracle, ro.trace) == case.expect, what  # this oracle run still takes the recorded branches
    assert rg.success, what
    assert rg.rtr_iterations == ro.outer_iters == len(case.expect), (what, rg)
    assert rg.rtr_accepted == sum(accepted), (what, rg)
    assert rg.latest_step_accepted == bool(accepted[-1]), (what, rg)
    assert rg.tcg_iterations == ro.tcg_iters, (what, rg)
    assert rg.tCGStatus == oracle.TCG_NAMES[ro.tCGStatus], (what, rg)
    op = oo.problem
    Xa = np.abs(X0).reshape(-1, case.r)
    scale = float((Xa * (abs(op.Qs) @ Xa)).sum())
    if p["G"] is not None:
        scale += float((np.abs(X0) * np.abs(p["G"])).sum())
    assert abs(rg.fInit - ro.fInit) <= 1e-14 * scale, what
    assert abs(rg.gradNormInit - ro.gradNormInit) <= 1e-10 * ro.gradNormInit, what
    assert abs(rg.fOpt - ro.fOpt) <= 1e-9 * abs(ro.fOpt) + 1e-14 * scale, what
    if case.kind in ("all-rejected", "give-up"):  # nothing was accepted: the input, bit for bit
        assert np.array_equal(np.ascontiguousarray(Xg).view(np.uint64), np.ascontiguousarray(X0).view(np.uint64)), what
        assert rg.rtr_accepted == 0 and not rg.latest_step_accepted and rg.fOpt == rg.fInit, (what, rg)
    else:
        assert relerr(Xg, Xo) < (1e-9 if case.kind == "shrink" else 1e-7), what


def solve_host(oracle, case, prob, run, tiny=None, **extra):
    import dpgo_amd
    X0, radius = run[0], run[1]
    opt = dpgo_amd.QuadraticOptimizer(prob, device_parameters(oracle, case, radius, tiny, **extra))
    Xg = matrix_to_tiles(opt.optimize(tiles_to_matrix(X0)), C.build_problem(oracle, case)["d"])
    return Xg, opt.getOptResult()


def check_launches(case, prob, one_launch, rg):
    info = prob.persistentInfo()
    if one_launch:  # (a one-launch solve that timed out fell back by itself: it fails here)
        assert info["enabled"] == 1 and info["last_members"] > 0, info
    else:
        assert info["last_members"] == 0, info
    assert rg.precond_used == case.precond, rg


def then_solve(oracle, case, prob, persistent, what):
    """After an all-rejected solve: an ordinary solve on the SAME handle from the same input matches the oracle (no trial
    point, no S of it, no quartered radius survives in the handle)."""
    nxt = C.by_name(case.then)
    run = oracle_window(oracle, nxt)
    assert np.array_equal(run[0], oracle_window(oracle, case)[0])
    Xg, rg = solve_host(oracle, nxt, prob, run)
    check_launches(nxt, prob, persistent, rg)
    check_result(oracle, nxt, rg, Xg, run, (what, "then", nxt.name))


def run_small(oracle, case, persistent, tiny=None):
    """A block-Jacobi / unpreconditioned case on the multi-launch scheme or the one-launch solve."""
    prob = device_problem(oracle, case)
    prob.setPersistent(persistent)
    run = oracle_window(oracle, case, tiny)
    Xg, rg = solve_host(oracle, case, prob, run, tiny)
    single = case.kind in ("shrink", "give-up")  # RTR_iterations == 1 keeps the multi-launch scheme whatever is requested
    check_launches(case, prob, persistent and not single, rg)
    check_result(oracle, case, rg, Xg, run, (case.name, "one-launch" if persistent else "multi-launch"))
    if case.then:
        then_solve(oracle, case, prob, persistent, case.name)
    return Xg, rg


def _ids(pairs):
    return ["%s/%s" % (c.name, p) for c, p in pairs]


SMALL = [(c, p) for c in CASES for p in c.paths if p in (MULTI, ONE)]


@pytest.mark.parametrize("case,path", SMALL, ids=_ids(SMALL))
def test_small_windows_on_both_schemes(oracle, case, path):
    """k_rtr_update + the host loop (multi-launch, just-in-time feed) and k_rtr_persist (one launch), block-Jacobi and no
    preconditioner, every (d, r): rejection after either boundary exit, every rho band, two rejections in a row, the
    radius clipped at Delta_max, all steps rejected (the returned iterate bitwise the input, then an ordinary solve on
    the same handle), and the single-iteration radius-shrink loop -- 3 - 5 tries, and twelve tries then the input back --
    which must stay on the multi-launch scheme although the one-launch solve is requested."""
    if case.kind in ("shrink", "give-up"):
        X1, r1 = run_small(oracle, case, False)
        X2, r2 = run_small(oracle, case, True)  # requested, not used (check_launches)
        assert np.array_equal(X1, X2) and (r1.tcg_iterations, r1.rtr_iterations, r1.fOpt) == (r2.tcg_iterations, r2.rtr_iterations, r2.fOpt)
        return
    run_small(oracle, case, path == ONE)


POLLED = [(c, POLL) for c in CASES if POLL in c.paths]


@pytest.mark.parametrize("case,path", POLLED, ids=_ids(POLLED))
def test_polling_feed_is_bitwise_the_just_in_time_feed(oracle, case, path):
    run_polled(oracle, case)


def run_polled(oracle, case, tiny=None):
    prob = device_problem(oracle, case)
    prob.setPersistent(False)
    run = oracle_window(oracle, case, tiny)
    Xj, rj = solve_host(oracle, case, prob, run, tiny)
    Xp, rp = solve_host(oracle, case, prob, run, tiny, tcg_poll_interval=1)
    check_launches(case, prob, False, rp)
    check_result(oracle, case, rp, Xp, run, (case.name, "polling"))
    assert np.array_equal(Xp, Xj)
    assert (rp.tcg_iterations, rp.rtr_iterations, rp.rtr_accepted, rp.latest_step_accepted, rp.tCGStatus, rp.fOpt) == (
        rj.tcg_iterations, rj.rtr_iterations, rj.rtr_accepted, rj.latest_step_accepted, rj.tCGStatus, rj.fOpt)


WITH_G = [(c, LINEAR) for c in CASES if LINEAR in c.paths]


@pytest.mark.parametrize("case,path", WITH_G, ids=_ids(WITH_G))
def test_linear_term_windows(oracle, case, path):
    """f = 0.5 <X Q, X> + <X, G> (dpgo_problem_set_G): the rho test's f1 carries the linear term; both schemes."""
    for persistent in (False, True):
        run_small(oracle, case, persistent)


PRECONDITIONED = [(c, p) for c in CASES for p in c.paths if p in (ADD1, ADD2, VCYCLE)]


@pytest.mark.parametrize("case,path", PRECONDITIONED, ids=_ids(PRECONDITIONED))
def test_preconditioned_windows(oracle, case, path):
    """The additive one-launch solve (aggregates on one and on two workgroup tiles) and the multi-launch loop around the
    V-cycle, on the hierarchy the handle builds, which is the one the table's oracle runs used."""
    run_preconditioned(oracle, case, path)


def run_preconditioned(oracle, case, path, tiny=None):
    prob = device_problem(oracle, case)
    ks = C.default_ks(oracle, case)
    if path == VCYCLE:
        assert prob.setupMultilevel()["ks"] == ks
    else:
        if path == ADD2:
            assert prob.additiveTiles(2) == 2
        plan = prob.additivePlan()
        assert plan["ks"] == ks and plan["lane_groups"] > 0, plan
    run = oracle_window(oracle, case, tiny)
    Xg, rg = solve_host(oracle, case, prob, run, tiny)
    info = prob.persistentInfo()
    assert rg.precond_used == case.precond, rg
    if path == VCYCLE:
        assert info["last_members"] == 0, info
    else:
        assert (info["last_members"], info["last_split"]) == (plan["aggregates"], plan["lane_groups"]), info
        assert info["last_tiles"] == 2 or path == ADD1, info
    assert prob.multilevelInfo()["ks"] == ks
    check_result(oracle, case, rg, Xg, run, (case.name, path))


SYMMETRIC = [(c, p) for c in CASES for p in c.paths if p in (SYM, SYM_HOST)]


@pytest.mark.parametrize("case,path", SYMMETRIC, ids=_ids(SYMMETRIC))
def test_symmetric_storage_windows(oracle, case, path):
    """The multi-launch loop on the symmetric storage of Q, with its own outer-iteration kernels (DPGO_OUTER_SYM, the
    default) and with the outer iteration on the plain copy."""
    run_symmetric(oracle, case, path)


def run_symmetric(oracle, case, path, tiny=None):
    with library_options({} if path == SYM else {"DPGO_OUTER_SYM": "0"}):
        prob = device_problem(oracle, case)
        assert prob.setSpmmVariant("symmetric") == "symmetric"
        prob.setPersistent(False)
        run = oracle_window(oracle, case, tiny)
        Xg, rg = solve_host(oracle, case, prob, run, tiny)
        assert prob.tcgKernelInfo()["symmetric"]
        check_launches(case, prob, False, rg)
        check_result(oracle, case, rg, Xg, run, (case.name, path))
        del prob


ENTERED = [(c, p) for c in CASES for p in c.paths if p in ENTRIES]


@pytest.mark.parametrize("persistent", [False, True], ids=["multi-launch", "one-launch"])
@pytest.mark.parametrize("case,path", ENTERED, ids=_ids(ENTERED))
def test_device_entries(oracle, case, path, persistent):
    """optimizeDevice, optimizeDeviceBegin / End and optimize_device_many (two handles at once) solve in the caller's
    buffer, here between NaN guards: after an all-rejected solve the buffer is bitwise the input (k_persist_commit leaves
    early, dpgo_optimize_device iterates in the caller's buffer), and an ordinary solve on the same handle follows."""
    run_entry(oracle, case, path, persistent)


def run_entry(oracle, case, path, persistent, tiny=None):
    import torch
    from dpgo_amd.solver import optimize_device_many
    import dpgo_amd
    p = C.build_problem(oracle, case)
    run = oracle_window(oracle, case, tiny)
    X0, radius = run[0], run[1]
    guard = guard_of(p["d"], case.r)
    probs = [device_problem(oracle, case) for _ in range(2 if path == MANY else 1)]
    bufs, images, opts = [], [], []
    for prob in probs:
        prob.setPersistent(persistent)
        bufs.append(Guarded(X0.size, guard, device=True, body=X0, guard_nan=True))
        images.append(bufs[-1].buf.cpu().numpy().view(np.uint64).copy())
        opts.append(dpgo_amd.QuadraticOptimizer(prob, device_parameters(oracle, case, radius, tiny)))
    if path == DEVICE:
        results = [opts[0].optimizeDevice(bufs[0].body)]
    elif path == BEGIN_END:
        opts[0].optimizeDeviceBegin(bufs[0].body)
        results = [opts[0].optimizeDeviceEnd()]
    else:
        results = optimize_device_many(opts, [b.body for b in bufs])
    torch.cuda.synchronize()
    for prob, buf, image, rg in zip(probs, bufs, images, results):
        now = buf.buf.cpu().numpy().view(np.uint64)
        assert np.array_equal(now[:guard], image[:guard]) and np.array_equal(now[guard + X0.size:], image[guard + X0.size:])
        if case.kind == "all-rejected":
            assert np.array_equal(now, image), (case.name, path)
        Xg = now[guard:guard + X0.size].view(np.float64).reshape(X0.shape).copy()
        check_launches(case, prob, persistent, rg)
        check_result(oracle, case, rg, Xg, run, (case.name, path, persistent))
        if case.then:
            then_solve(oracle, case, prob, persistent, (case.name, path))


def _first_rejecting(paths):
    return next(c for c in CASES if c.kind == "window" and set(paths) & set(c.paths) and any(e[2] == REJ for e in c.expect))


@pytest.mark.parametrize("path", [MULTI, POLL, ONE, LINEAR, ADD1, ADD2, VCYCLE, SYM, SYM_HOST, DEVICE, BEGIN_END, MANY])
def test_without_the_tiny_decrease_clause(oracle, path):
    """accept_tiny_decrease = False on both sides (the flag reaches k_rtr_begin and the one-launch solve's RtrArgs; the
    device entries fill their own parameter record): one rejecting window per path, same assertions."""
    case = _first_rejecting([path])
    if path in (MULTI, ONE):
        run_small(oracle, case, path == ONE, tiny=False)
    elif path == POLL:
        run_polled(oracle, case, tiny=False)
    elif path == LINEAR:
        for persistent in (False, True):
            run_small(oracle, case, persistent, tiny=False)
    elif path in (SYM, SYM_HOST):
        run_symmetric(oracle, case, path, tiny=False)
    elif path in ENTRIES:
        for persistent in (False, True):
            run_entry(oracle, case, path, persistent, tiny=False)
    else:
        run_preconditioned(oracle, case, path, tiny=False)
