"""tCG's residual carries H eta: r = g + H eta at every exit, the boundary step included (oracle only, no device).

The device's rho test takes <eta, H eta> from the vectors tCG leaves behind, <eta, r - g>, instead of applying the Hessian to
eta once more (k_retract).  That rests on two things, pinned here independently of any kernel:

  * the recurrences: r = g at the start, r += alpha H delta beside eta += alpha delta, H delta advanced by
    H delta' = beta H delta - H z as the device does it (k_tcg_hess*), so r - g is H applied to eta up to round-off;
  * the boundary step: tCG's two boundary exits (EXCREGION, NEGCURVTURE) end with eta += tau delta, and r has to follow with
    r += tau H delta (k_tcg_update*; ROPTLIB leaves r stale there because nothing reads it afterwards).

`device_tcg` restates the loop with that boundary update; up to it, it is the oracle's tcg(hess_recurrence=True) statement
for statement, which the tests assert bit for bit.  The bound is relative to |eta| |H eta|: 1e-10 leaves four digits over
what 50 unpreconditioned iterations (the longest run of the recurrences the device's default budget allows, and the
largest drift) accumulate in fp64.
"""
import math

import numpy as np
import pytest

import trust_region_cases as C

RTOL = 1e-10
DR = [(2, 2), (2, 4), (3, 3), (3, 5)]
PRECONDS = ["none", "jacobi"]
POSES = {(2, 2): 30, (2, 4): 41, (3, 3): 52, (3, 5): 60}

_PROBLEMS = {}


def device_tcg(oracle, p, X, g, S, Delta, max_inner, theta=1.0, kappa=0.1):
    """tCG as the device runs it; returns (eta, r, status, products)."""
    dot = oracle.dot
    r = g.copy()
    eta = np.zeros_like(g)
    e_Pe = e_Pd = 0.0
    norm_r0 = math.sqrt(dot(r, r))
    z = p.precondition(X, r)
    z_r = dot(z, r)
    d_Pd = z_r
    delta = -z
    status, j, products, beta, Hd = oracle.TCG_MAXITER, 0, 0, 0.0, None
    while j < max_inner:
        Hz = p.rie_hess(X, S, z)
        Hd = -Hz if j == 0 else beta * Hd - Hz
        products += 1
        d_Hd = dot(delta, Hd)
        alpha = z_r / d_Hd if d_Hd != 0 else math.inf
        e_Pe_new = e_Pe + 2.0 * alpha * e_Pd + alpha * alpha * d_Pd
        if d_Hd <= 0 or e_Pe_new >= Delta * Delta:
            tau = (-e_Pd + math.sqrt(e_Pd * e_Pd + d_Pd * (Delta * Delta - e_Pe))) / d_Pd
            eta = eta + tau * delta
            r = r + tau * Hd  # the boundary step carries the residual along
            status = oracle.TCG_NEGCURV if d_Hd < 0 else oracle.TCG_EXCREGION
            break
        e_Pe = e_Pe_new
        eta = eta + alpha * delta
        r = r + alpha * Hd
        norm_r = math.sqrt(dot(r, r))
        if norm_r <= norm_r0 * min(norm_r0 ** theta, kappa):
            status = oracle.TCG_LCON if kappa < norm_r0 ** theta else oracle.TCG_SCON
            break
        z = p.precondition(X, r)
        z_r, zold_rold = dot(z, r), z_r
        beta = z_r / zold_rold
        delta = beta * delta - z
        e_Pd = beta * (e_Pd + alpha * d_Pd)
        d_Pd = z_r + beta * beta * d_Pd
        j += 1
    return eta, r, status, products


def problem(oracle, d, r):
    """(Q, ground truth) of a random graph of 30-60 poses (chain, loop closures, a hub row), cached."""
    from test_parity_gpu import _random_graph
    if (d, r) not in _PROBLEMS:
        n = POSES[(d, r)]
        om, T, _ = _random_graph(oracle, d, n, n // 2, 6, seed=90 + n)
        _PROBLEMS[(d, r)] = (oracle.construct_Q(n, d, om), T)
    return _PROBLEMS[(d, r)]


def at_point(oracle, p, X):
    EG = p.euc_grad(X)
    return oracle.tangent_project(X, EG, p.d), p.sym_ytg(X, EG)


def check_exit(oracle, p, X, Delta, max_inner, what, kappa=0.1):
    """Runs tCG from X; asserts the identity at its exit and returns (status name, products)."""
    g, S = at_point(oracle, p, X)
    eta, r, status, products = device_tcg(oracle, p, X, g, S, Delta, max_inner, kappa=kappa)
    eta_o, status_o, _, products_o = oracle.tcg(p, X, g, S, Delta, max_inner, kappa=kappa, hess_recurrence=True)
    assert np.array_equal(eta, eta_o) and (status, products) == (status_o, products_o), what  # the restatement is the oracle's
    Heta = p.rie_hess(X, S, eta)
    got, want = oracle.dot(eta, r - g), oracle.dot(eta, Heta)
    bound = RTOL * np.linalg.norm(eta) * np.linalg.norm(Heta)
    print("%s: %s after %d products, <eta, r - g> - <eta, H eta> = %.3e, bound %.3e" % (
        what, oracle.TCG_NAMES[status], products, got - want, bound))
    assert abs(got - want) <= bound, (what, got, want, bound)
    # the model decrease the rho test divides by, both ways
    assert abs(oracle.dot(eta, g + 0.5 * Heta) - 0.5 * (oracle.dot(eta, g) + oracle.dot(eta, r))) <= 0.5 * bound, what
    return oracle.TCG_NAMES[status], products


def starts(oracle, d, r):
    """far: the random start of the trust-region table (negative curvature, the boundary); near: the ground truth with
    noise (positive curvature: tCG runs until its budget or its residual test ends it); tight: a few outer iterations
    further, where |g| < kappa and the superlinear clause of the residual test is the one that holds."""
    from test_parity_gpu import random_point
    Q, T = problem(oracle, d, r)
    n = Q.n
    rng = np.random.default_rng(11)
    near = oracle.polar_project(oracle.lift(T, r) + 0.02 * rng.standard_normal((n, d + 1, r)), d)
    oo = oracle.QuadraticOptimizer(oracle.QuadraticProblem(Q, None, r, d, precond="jacobi"),
                                   oracle.ROptParameters(RTR_iterations=6, RTR_tCG_iterations=200, gradnorm_tol=1e-3))
    far = {"far%d" % seed: random_point(oracle, n, d, r, seed) for seed in (4, 5, 7)}
    return dict(far=random_point(oracle, n, d, r, 3), near=near, tight=oo.optimize(near), **far)


@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("d,r", DR)
def test_residual_holds_H_eta_at_every_exit(oracle, d, r, precond):
    Q, _ = problem(oracle, d, r)
    p = oracle.QuadraticProblem(Q, None, r, d, precond=precond)
    X = starts(oracle, d, r)
    what = lambda s: "(%d, %d) %s, %s" % (d, r, precond, s)
    seen = set()
    # both boundary exits: the table's start and radii, a radius small enough to bind before the curvature turns, and one
    # that binds after some interior steps
    for Delta in (1e3, 1.0, 1e-2):
        seen.add(check_exit(oracle, p, X["far"], Delta, 50, what("far, radius %g" % Delta))[0])
    for seed in (4, 5, 7):  # (the table's other random starts)
        seen.add(check_exit(oracle, p, X["far%d" % seed], 1e3, 50, what("far, seed %d" % seed))[0])
    for Delta in (0.3, 0.05):
        seen.add(check_exit(oracle, p, X["near"], Delta, 50, what("near, radius %g" % Delta))[0])
    # the budget
    status, products = check_exit(oracle, p, X["near"], 1e6, 3, what("near, 3 products"))
    assert (status, products) == (C.MAXIT, 3)
    seen.add(status)
    # the residual test: its linear clause from the noisy start, its superlinear one close to the optimum
    seen.add(check_exit(oracle, p, X["near"], 1e6, 400, what("near, to convergence"))[0])
    seen.add(check_exit(oracle, p, X["tight"], 1e6, 400, what("tight, to convergence"))[0])
    # no product at all: eta = 0, r = g
    assert check_exit(oracle, p, X["near"], 1e6, 0, what("no budget")) == (C.MAXIT, 0)
    assert seen == {C.NEGC, C.EXCR, C.MAXIT, C.LCON, C.SCON}, (what("exits"), seen)


@pytest.mark.parametrize("d,r", DR)
def test_fifty_unpreconditioned_iterations(oracle, d, r):
    """The longest run of the recurrences the default budget allows, without a preconditioner: the largest drift between
    r - g and H eta.  (kappa = 1e-300 switches the residual test off, which would end these runs after 7 - 8 products: the
    recurrences go on past convergence, down to the round-off floor of r.)"""
    Q, _ = problem(oracle, d, r)
    p = oracle.QuadraticProblem(Q, None, r, d, precond="none")
    status, products = check_exit(oracle, p, starts(oracle, d, r)["near"], 1e6, 50, "(%d, %d) none, 50 products" % (d, r),
                                  kappa=1e-300)
    assert (status, products) == (C.MAXIT, 50)
