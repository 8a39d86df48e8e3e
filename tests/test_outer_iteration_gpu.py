"""The tail of the multi-launch outer iteration: the rho test from tCG's residual, acceptance without copying g and S.

Two things changed there and each has a way to go wrong that the parity suite would only show as a slightly different
trajectory:

  * <eta, H eta> and <eta, g> come from k_retract's sums over tCG's residual (r = g + H eta, tests/test_rho_identity_cpu.py)
    instead of a second pass over Q.  DPGO_RHO_EXACT=1 keeps that pass (k_hess) as the reference path: on windows whose
    every rho is at least RHO_MARGIN from a threshold both take the same decisions and radii, so everything that follows is
    the same arithmetic -- iterates and results are compared BIT FOR BIT, on every feed mode / storage / preconditioner of
    the multi-launch scheme and after every tCG exit.
  * k_rtr_update leaves g and S where they are and the host exchanges the roles of (g1, S1) and (g2, S2) behind every
    launch; after a rejection, and in an iteration the device skips because the solve has already stopped, the kernel
    copies the current pair across instead.  A handle therefore sees odd and even numbers of exchanges, rejections between
    them and skipped iterations: sequences of solves on ONE handle, each against the oracle, through the host entry and
    through optimizeDevice in a caller buffer between NaN guards.

The windows are those of tests/trust_region_cases.py (same problems, starts and radii); where a test needs another length
or tCG budget than the table has, the case is derived here and its branches and rho margins are asserted on the oracle's
run before the device is compared with it.
"""
import dataclasses

import numpy as np
import pytest

import trust_region_cases as C
from conftest import device_tcg_mode
from test_launch_geometry_gpu import Guarded, guard_of, library_options
from test_parity_gpu import relerr
from test_trust_region_branches_gpu import (check_result, device_parameters, device_problem, oracle_window, solve_host)
from trust_region_cases import (ACC, CASES, EXCR, HI, LCON, LINEAR, MAXIT, MID, MULTI, NEGC, POLL, REJ, SCON, SYM, SYM_HOST,
                                VCYCLE, Case)

pytestmark = pytest.mark.gpu

FIELDS = ("rtr_iterations", "rtr_accepted", "latest_step_accepted", "tcg_iterations", "tCGStatus", "fOpt")
_RUNS = {}


def margins_hold(trace):
    return all(abs(t["rho"] - thr) >= C.RHO_MARGIN for t in trace for thr in (0.1, 0.25, 0.75))


def own_window(oracle, case):
    """The oracle on a case that is not in the table (cached); its branches are the ones the case records and every rho
    keeps the table's margin."""
    if case.name not in _RUNS:
        p = C.build_problem(oracle, case)
        run = C.run_window(oracle, case, hess_recurrence=device_tcg_mode(p["n"], p["d"], case.r))
        trace = run[2].result.trace
        assert C.observed(oracle, trace) == case.expect, (case.name, C.observed(oracle, trace))
        assert margins_hold(trace), (case.name, [t["rho"] for t in trace])
        _RUNS[case.name] = run
    return _RUNS[case.name]


def window_of(oracle, case):
    return oracle_window(oracle, case) if case in CASES else own_window(oracle, case)


# tCG exits the table does not have (its windows start far from an optimum and end on the boundary): the budget, and the
# two clauses of the residual test
EXIT_CASES = [
    Case('maxiter-2-3-jacobi-k7', ('random', 2, False), 3, 'jacobi', ('random', 3), 1e3, 7,
         ((MAXIT, HI, ACC), (MAXIT, MID, ACC), (MAXIT, HI, ACC),),
         (MULTI,), tcg_iterations=5, trajectory=12),  # rho 0.978 0.307 0.916
    Case('converging-tinyGrid3D-4-k2', ('data', 'tinyGrid3D'), 4, 'jacobi', ('chordal',), 100.0, 2,
         ((LCON, HI, ACC), (SCON, HI, ACC),),
         (MULTI,), tcg_iterations=100),  # rho 1.000 1.000
]


def _first(path, kind="window"):
    """The table's first case of that kind on that path (a window: one with a rejection in it)."""
    return next(c for c in CASES if c.kind == kind and path in c.paths and (kind != "window" or any(e[2] == REJ for e in c.expect)))


BITWISE = [(_first(MULTI), MULTI), (_first(POLL), POLL), (_first(LINEAR), LINEAR), (_first(VCYCLE), VCYCLE),
           (_first(SYM), SYM), (_first(SYM_HOST), SYM_HOST),
           (_first(MULTI, "shrink"), MULTI), (_first(MULTI, "give-up"), MULTI), (_first(MULTI, "all-rejected"), MULTI),
           # (both boundary exits in 3-D -- the span kernels' boundary step; the 2-D cases with odd r above run the generic ones)
           (C.by_name('random-3-5-jacobi-k3'), MULTI), (C.by_name('random-3-4-jacobi-k0'), MULTI)] + [(c, MULTI) for c in EXIT_CASES]


def solve_on_path(oracle, case, path, run, env):
    """One solve of the window on `path` of the multi-launch scheme under the library switches `env`."""
    if path == SYM_HOST:
        env = dict(env, DPGO_OUTER_SYM="0")
    with library_options(env):
        prob = device_problem(oracle, case)
        prob.setPersistent(False)
        if path == VCYCLE:
            assert prob.setupMultilevel()["ks"] == C.default_ks(oracle, case)
        if path in (SYM, SYM_HOST):
            assert prob.setSpmmVariant("symmetric") == "symmetric"
        Xg, rg = solve_host(oracle, case, prob, run, **({"tcg_poll_interval": 1} if path == POLL else {}))
        assert prob.persistentInfo()["last_members"] == 0 and rg.precond_used == case.precond, (case.name, path, rg)
        if path in (SYM, SYM_HOST):
            assert prob.tcgKernelInfo()["symmetric"]
        del prob
    return Xg, rg


@pytest.mark.parametrize("case,path", BITWISE, ids=["%s/%s" % (c.name, p) for c, p in BITWISE])
def test_residual_rho_is_bitwise_the_reference_path(oracle, case, path):
    """DPGO_RHO_EXACT=1 (k_hess in the tail) against the default (k_retract's sums): same iterates, bit for bit, same
    result record; the product counts say which path ran."""
    run = window_of(oracle, case)
    assert margins_hold(run[2].result.trace), case.name
    Xe, re_ = solve_on_path(oracle, case, path, run, {"DPGO_RHO_EXACT": "1"})
    Xd, rd = solve_on_path(oracle, case, path, run, {})
    assert np.array_equal(Xe.view(np.uint64), Xd.view(np.uint64)), (case.name, path, relerr(Xd, Xe))
    assert all(getattr(re_, f) == getattr(rd, f) for f in FIELDS), (case.name, path, re_, rd)
    assert rd.spmm_count == 1 + rd.rtr_iterations + rd.tcg_iterations, rd
    assert re_.spmm_count == 1 + 2 * re_.rtr_iterations + re_.tcg_iterations, re_
    check_result(oracle, case, rd, Xd, run, (case.name, path))
    exits = {e[0] for c, _ in BITWISE for e in c.expect}
    assert exits == {NEGC, EXCR, MAXIT, LCON, SCON}, exits  # (the table as selected here has one window per tCG exit)


# ---------------------------------------------------------------------------------------------- buffer roles
REJECT_THEN_ACCEPT = C.by_name('random-2-3-jacobi-k2')  # rho 0.053 0.904, then 0.567 0.667 (the trajectory's iterations 4, 5)
ALL_REJECTED = C.by_name('all-rejected-2-3-jacobi')  # (the same problem)


def derived(case, k, expect, **kw):
    return dataclasses.replace(case, name="%s@k%d x%d" % (case.name, k, len(expect)), k=k, expect=expect, **kw)


def sequence():
    """(case, stop?) solved back to back on one handle: 2, 3 and 4 exchanges of the buffer roles after a rejection, an
    accepting window, nothing accepted at all, a solve that stops after its first accepted step of three (the host may have
    enqueued the next iteration, which the device then skips), and an ordinary solve behind it."""
    tail = ((EXCR, MID, ACC), (EXCR, MID, ACC))
    steps = [(derived(REJECT_THEN_ACCEPT, 2, REJECT_THEN_ACCEPT.expect + tail[:extra]), False) for extra in (0, 1, 2)]
    accepting = derived(REJECT_THEN_ACCEPT, 3, ((EXCR, HI, ACC),) + tail)
    return steps + [(accepting, False), (ALL_REJECTED, False), (accepting, True), (steps[0][0], False)]


def stopping_run(oracle, case):
    """The oracle on an accepting window with gradnorm_tol between the gradient norms in front of and behind its first step:
    one outer iteration of the three, then the stop.  Returns (X0, radius, optimizer, Xopt, tol)."""
    key = (case.name, "stop")
    if key not in _RUNS:
        X0, radius, oo, _ = own_window(oracle, case)
        ngf = [t["ngf"] for t in oo.result.trace]
        assert oo.result.trace[0]["accept"] and ngf[1] < 0.9 * ngf[0], ngf
        tol = float(np.sqrt(ngf[0] * ngf[1]))
        p = C.build_problem(oracle, case)
        prm = oracle.ROptParameters(verbose=True, gradnorm_tol=tol, **C.window_parameters(oracle, case, radius))
        stopped = oracle.QuadraticOptimizer(C.oracle_problem(oracle, case), prm, accept_tiny_decrease=case.tiny,
                                            hess_recurrence=device_tcg_mode(p["n"], p["d"], case.r))
        Xs = stopped.optimize(X0)
        assert stopped.result.outer_iters == 1 and prm.RTR_iterations == 3, stopped.result
        _RUNS[key] = (X0, radius, stopped, Xs, tol)
    return _RUNS[key]


def check_stopped(oracle, rg, Xg, run, what):
    _, _, oo, Xo, tol = run
    ro = oo.result
    assert rg.success and (rg.rtr_iterations, rg.rtr_accepted, rg.latest_step_accepted) == (1, 1, True), (what, rg)
    assert rg.tcg_iterations == ro.tcg_iters and rg.tCGStatus == oracle.TCG_NAMES[ro.tCGStatus], (what, rg)
    assert rg.gradNormOpt < tol and abs(rg.fOpt - ro.fOpt) <= 1e-9 * abs(ro.fOpt), (what, rg, ro.fOpt)
    assert relerr(Xg, Xo) < 1e-7, what


def device_solve(case, opt, X0, d, r):
    """optimizeDevice in a caller buffer between NaN guards: (iterate, result); the guards are untouched, and so is the
    iterate when nothing was accepted."""
    import torch
    guard = guard_of(d, r)
    buf = Guarded(X0.size, guard, device=True, body=X0, guard_nan=True)
    image = buf.buf.cpu().numpy().view(np.uint64).copy()
    rg = opt.optimizeDevice(buf.body)
    torch.cuda.synchronize()
    now = buf.buf.cpu().numpy().view(np.uint64)
    assert np.array_equal(now[:guard], image[:guard]) and np.array_equal(now[guard + X0.size:], image[guard + X0.size:]), case.name
    if case.kind == "all-rejected":
        assert np.array_equal(now, image), case.name
    return now[guard:guard + X0.size].view(np.float64).reshape(X0.shape).copy(), rg


@pytest.mark.parametrize("feed", ["just-in-time", "polling"])
@pytest.mark.parametrize("entry", ["optimize", "optimizeDevice"])
def test_buffer_roles_across_solves_on_one_handle(oracle, entry, feed):
    """Every solve of the sequence against the oracle, on one handle.  (The polling feed always enqueues the iteration
    behind the stop: it reads the stop flag but not the progress word that would end the host loop early; the just-in-time
    feed does whenever its launches are ahead of the device.)"""
    import dpgo_amd
    steps = sequence()
    prob = device_problem(oracle, steps[0][0])
    prob.setPersistent(False)
    d = C.build_problem(oracle, steps[0][0])["d"]
    extra = {"tcg_poll_interval": 1} if feed == "polling" else {}
    for number, (case, stop) in enumerate(steps):
        what = (entry, feed, number, case.name, "stop" if stop else "")
        run = stopping_run(oracle, case) if stop else window_of(oracle, case)
        more = dict(extra, gradnorm_tol=run[4]) if stop else extra
        if entry == "optimize":
            Xg, rg = solve_host(oracle, case, prob, run, **more)
        else:
            opt = dpgo_amd.QuadraticOptimizer(prob, device_parameters(oracle, case, run[1], **more))
            Xg, rg = device_solve(case, opt, run[0], d, case.r)
        assert prob.persistentInfo()["last_members"] == 0, what
        if stop:
            check_stopped(oracle, rg, Xg, run, what)
        else:
            check_result(oracle, case, rg, Xg, run, what)
