"""tCG's kept directions: the multi-launch solve that writes delta_k into a ring and lets k_retract sum eta once, against
the path that adds alpha delta to eta every iteration (DPGO_TCG_DIRS=0, the reference path).

The retraction folds eta = fma(c_{K-1}, delta_{K-1}, ... fma(c_0, delta_0, +0)): the fused multiply-adds of the running sum,
in its order, on its operands.  Nothing else of the solve changes, so the two paths are compared BIT FOR BIT -- iterates on
their uint64 view, every field of the result record for equality -- and what can go wrong is the bookkeeping, which every
test below aims at:

  * the slot a Hessian-step kernel reads and writes follows the state record's iteration index, through every exit of tCG
    (negative curvature and the boundary: the coefficient is tau; the budget: the last slot; both clauses of the residual
    test, also raised one kernel early by the restriction), through a rejected step followed by a new run (the count starts
    at 0 again), the radius-shrink mode, the polling and the just-in-time feed, 2-D blocks with an odd tile (generic
    kernels) and 3-D blocks (span kernels, symmetric storage);
  * eta itself is materialised by the retraction: the DPGO_RHO_EXACT=1 tail (k_hess on p->eta) gives the same bits on both;
  * partial tiles, one tile, several tiles per workgroup under forced launch caps;
  * the ring's life: grown for a larger budget, kept for a smaller one, refused by DPGO_TCG_DIRS_MAX_MB=0 (the solve falls
    back and says so), released with the handle.

The windows are those of tests/test_outer_iteration_gpu.py (same cases, same oracle runs, cached there)."""
import ctypes as C
import gc

import numpy as np
import pytest

import trust_region_cases as TC
from test_device_memory_gpu import live
from test_launch_geometry_gpu import Handle, graph_Q, library_options, point, tile_poses
from test_outer_iteration_gpu import BITWISE, EXIT_CASES, FIELDS, margins_hold, window_of
from test_parity_gpu import relerr
from test_trust_region_branches_gpu import device_problem, solve_host
from trust_region_cases import EXCR, LCON, LINEAR, MAXIT, MULTI, NEGC, POLL, SCON, SYM, SYM_HOST, VCYCLE

pytestmark = pytest.mark.gpu

REFERENCE = {"DPGO_TCG_DIRS": "0"}
IDS = ["%s/%s" % (c.name, p) for c, p in BITWISE]


def solve_in_mode(oracle, case, path, run, env, deferred):
    """One solve of the window on `path` of the multi-launch scheme under the switches `env`: (iterate, result record).
    The handle reports the mode the solve was meant to run in, and a ring that holds the solve's tCG budget."""
    if path == SYM_HOST:
        env = dict(env, DPGO_OUTER_SYM="0")
    with library_options(env):
        prob = device_problem(oracle, case)
        prob.setPersistent(False)
        if path == VCYCLE:
            assert prob.setupMultilevel()["ks"] == TC.default_ks(oracle, case)
        if path in (SYM, SYM_HOST):
            assert prob.setSpmmVariant("symmetric") == "symmetric"
        Xg, rg = solve_host(oracle, case, prob, run, **({"tcg_poll_interval": 1} if path == POLL else {}))
        info = prob.tcgKernelInfo()
        assert prob.persistentInfo()["last_members"] == 0 and rg.precond_used == case.precond, (case.name, path, rg)
        assert info["directions"] == deferred, (case.name, path, env, info)
        if deferred:
            assert info["direction_slots"] >= max(1, case.tcg_iterations), (case.name, info)
        if path in (SYM, SYM_HOST):
            assert info["symmetric"]
        del prob
    return Xg, rg


def same_bits(a, b):
    """Equal as bit patterns (so a NaN equals itself): arrays of doubles, or result records given as tuples of numbers."""
    a, b = (np.ascontiguousarray(np.asarray(v, dtype=np.float64)) for v in (a, b))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("case,path", BITWISE, ids=IDS)
def test_kept_directions_are_bitwise_the_reference_path(oracle, case, path):
    """DPGO_TCG_DIRS=0 against the default on every multi-launch path and after every exit of tCG."""
    run = window_of(oracle, case)
    assert margins_hold(run[2].result.trace), case.name
    Xr, rr = solve_in_mode(oracle, case, path, run, REFERENCE, False)
    Xd, rd = solve_in_mode(oracle, case, path, run, {}, True)
    assert same_bits(Xr, Xd), (case.name, path, relerr(Xd, Xr))
    assert all(getattr(rr, f) == getattr(rd, f) for f in FIELDS + ("fInit", "gradNormInit", "gradNormOpt", "spmm_count")), (rr, rd)
    exits = {e[0] for c, _ in BITWISE for e in c.expect}
    assert exits == {NEGC, EXCR, MAXIT, LCON, SCON}, exits
    assert {p for _, p in BITWISE} >= {MULTI, POLL, LINEAR, VCYCLE, SYM, SYM_HOST}


@pytest.mark.parametrize("case,path", BITWISE, ids=IDS)
def test_exact_tail_reads_the_materialised_eta(oracle, case, path):
    """DPGO_RHO_EXACT=1 applies H to p->eta after the retraction: the eta the retraction wrote from the ring is, bit for
    bit, the running sum of the reference path -- or rho, the radii and every later iterate would differ."""
    run = window_of(oracle, case)
    Xr, rr = solve_in_mode(oracle, case, path, run, dict(REFERENCE, DPGO_RHO_EXACT="1"), False)
    Xd, rd = solve_in_mode(oracle, case, path, run, {"DPGO_RHO_EXACT": "1"}, True)
    assert same_bits(Xr, Xd), (case.name, path, relerr(Xd, Xr))
    assert all(getattr(rr, f) == getattr(rd, f) for f in FIELDS + ("spmm_count",)), (rr, rd)
    assert rd.spmm_count == 1 + 2 * rd.rtr_iterations + rd.tcg_iterations, rd  # (the exact tail ran)


def test_polling_feed_and_radius_shrink_mode(oracle):
    """The selection above holds one window fed at tcg_poll_interval = 1 and one solved with RTR_iterations = 1 (the radius
    is quartered until a step is accepted: several tCG runs, each starting its count at 0)."""
    polled = [c for c, p in BITWISE if p == POLL]
    shrink = [c for c, p in BITWISE if c.kind == "shrink"]
    assert polled and shrink
    for case in shrink:
        assert TC.window_parameters(oracle, case, 1.0)["RTR_iterations"] == 1 and len(case.expect) > 1, case.name
    budget = [c for c in EXIT_CASES if any(e[0] == MAXIT for e in c.expect)]
    assert budget and all((c, MULTI) in BITWISE for c in budget)  # (a run that ends on its budget writes the last slot)


# ---------------------------------------------------------------------------------------------- raw handles
RAW = ("success", "fInit", "gradNormInit", "fOpt", "gradNormOpt", "tCGStatus", "rtr_iterations", "rtr_accepted",
       "tcg_iterations", "spmm_count", "latest_step_accepted", "precond_used")


def raw_solve(h, X0, budget, outer=3, radius=10.0):
    """dpgo_optimize on a Handle (block-Jacobi, tiles in and out): (iterate, result fields, (deferred, slots))."""
    L, lib = h.L, h.lib
    cp, cr = L.RoptParamsC(), L.RoptResultC()
    lib.dpgo_ropt_params_default(C.byref(cp))
    cp.precond, cp.RTR_iterations, cp.RTR_tCG_iterations, cp.RTR_initial_radius = L.PRECOND_BLOCK_JACOBI, outer, budget, radius
    cp.gradnorm_tol = 1e-12
    X = np.ascontiguousarray(X0)
    out = np.full_like(X, np.nan)
    L.check(lib.dpgo_optimize(h.h, C.byref(cp), L.ptr(X), L.ptr(out), C.byref(cr)))
    deferred, slots = C.c_int(-1), C.c_int(-1)
    L.check(lib.dpgo_problem_tcg_directions_info(h.h, C.byref(deferred), C.byref(slots)))
    return out, tuple(getattr(cr, f) for f in RAW), (deferred.value, slots.value)


D3, R5 = 3, 5
P = tile_poses(D3, 1)


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("storage", ["split4", "symmetric"])
def test_tile_edges_under_forced_caps(oracle, cap, storage):
    """n = 1, P - 1, P, P + 1, 17 P + 3 at d = 3, r = 5 with the update, Hessian-step and retraction grids capped at 1 and
    3 workgroups: partial tiles and several tiles per workgroup in the slot addressing and in the retraction's sum, on
    k_tcg_hess_span (four lane groups per pose) and on the symmetric storage's kernel."""
    caps = {k: str(cap) for k in ("DPGO_GRID_UPDATE", "DPGO_GRID_HESS", "DPGO_GRID_HESS_SYM", "DPGO_GRID_RETRACT")}
    caps["DPGO_PERSIST"] = "0"
    if storage == "symmetric":
        caps.update(DPGO_SPLIT="1", DPGO_SPMM_SYMMETRIC="1")
    for n in (1, P - 1, P, P + 1, 17 * P + 3):
        Qb, T = graph_Q(oracle, D3, n)
        X0 = point(oracle, T, D3, R5, seed=n)[0]
        got = {}
        for name, env in (("reference", dict(caps, **REFERENCE)), ("deferred", caps)):
            with library_options(env) as lib:
                h = Handle(lib, Qb, R5, D3)
                try:
                    got[name] = raw_solve(h, X0, budget=6)
                finally:
                    h.close()
        (Xr, rr, mr), (Xd, rd, md) = got["reference"], got["deferred"]
        assert mr == (0, 0) and md == (1, 6), (n, mr, md)
        assert not np.isnan(Xd).any() and (n == 1 or rd[RAW.index("tcg_iterations")] > 0), (n, rd)
        assert same_bits(Xr, Xd), (n, cap, storage, relerr(Xd, Xr))
        assert same_bits(rr, rd), (n, rr, rd)


def test_ring_life_cycle(oracle):
    """One handle, tCG budgets 3, 7, 3: the ring is allocated by the first deferred solve, grown for the larger budget and
    kept for the smaller one, each solve bitwise the reference path's; under DPGO_TCG_DIRS_MAX_MB=0 the solve falls back,
    reports the reference mode and gives the same bits; with RTR_tCG_iterations = 0 eta is zero and the iterate is
    retracted onto itself on both paths; after the destroy the library holds what it held before the handle."""
    n = P + 1
    Qb, T = graph_Q(oracle, D3, n)
    X0 = point(oracle, T, D3, R5, seed=5)[0]
    budgets = (3, 7, 3, 0)
    base_env = {"DPGO_PERSIST": "0"}
    with library_options(dict(base_env, **REFERENCE)) as lib:
        h = Handle(lib, Qb, R5, D3)
        try:
            reference = [raw_solve(h, X0, b) for b in budgets]
        finally:
            h.close()
    assert all(m == (0, 0) for _, _, m in reference)
    gc.collect()
    base = live()
    with library_options(base_env) as lib:
        h = Handle(lib, Qb, R5, D3)
        try:
            created = live()
            slots = []
            for b, (Xr, rr, _) in zip(budgets, reference):
                Xd, rd, md = raw_solve(h, X0, b)
                assert md[0] == 1 and same_bits(Xr, Xd) and same_bits(rr, rd), (b, md, rr, rd)
                slots.append(md[1])
            assert slots == [3, 7, 7, 7], slots
            assert live()[0] == created[0] + 2  # (the ring and its step lengths)
            assert live()[1] - created[1] == 8 * (7 * n * (D3 + 1) * R5 + 7 + 1)
            # a budget the ring may not hold: the reference path, same bits, the ring stays as it is
            with library_options(dict(base_env, DPGO_TCG_DIRS_MAX_MB="0")):
                Xd, rd, md = raw_solve(h, X0, 7)
                assert md == (0, 7) and same_bits(reference[1][0], Xd) and same_bits(reference[1][1], rd), (md, rd)
            Xd, rd, md = raw_solve(h, X0, 7)  # (the outer switches are back)
            assert md == (1, 7) and same_bits(reference[1][0], Xd) and same_bits(reference[1][1], rd), (md, rd)
        finally:
            h.close()
    assert live() == base
