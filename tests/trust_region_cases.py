"""Case table for the trust-region branches the data-set parity tests never take (a plain module, no tests).

The tail of ROPTLIB's SolversTR::Run -- rho test, radius update, accept / reject, tCG's two boundary exits -- exists
several times on the device (k_rtr_update + the host loop of solve.hip, k_rtr_persist, the loops around the V-cycle and
the symmetric-storage kernels).  From a chordal start every step of every data set is accepted with rho > 0.75, so the
cases here start far from any optimum: random points on random graphs, large initial radii.

Far from an optimum, through negative curvature, round-off between two summation orders grows from one outer iteration
to the next, so the unit of comparison is a WINDOW: the oracle runs a long trajectory (`radius`, `TRAJECTORY` outer
iterations) from the case's start; the window starts at that trajectory's iterate x_k with RTR_initial_radius = Delta_k
(the radius in front of iteration k) and runs `len(expect)` outer iterations, freshly, on both sides.  x_k is recomputed
by the oracle whenever a test runs.  `expect` records what the case is there for: (tCG exit, rho band, decision) per
iteration of its window; tests/test_trust_region_cases_cpu.py checks it, the margins of every rho to the thresholds
0.1 / 0.25 / 0.75, and that the table as a whole keeps every (path, branch) pair.
"""
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

from conftest import DATA

DR = [(2, 2), (2, 3), (2, 4), (2, 5), (3, 3), (3, 4), (3, 5), (3, 6)]  # DPGO_FOR_DR (csrc/host.h)
TRAJECTORY = 8  # outer iterations of the trajectory the windows are cut from
RHO_MARGIN = 0.01  # every rho of a window is at least this far from 0.1, 0.25 and 0.75
NEGCURV_MARGIN = 1e-6  # NEGCURVTURE: d_Hd <= -NEGCURV_MARGIN |delta| |H delta|

LO, MID, HI = "rho<0.25", "0.25<=rho<=0.75", "rho>0.75"
ACC, REJ = "accepted", "rejected"
NEGC, EXCR, LCON, SCON, MAXIT = "NEGCURVTURE", "EXCREGION", "LCON", "SCON", "MAXITER"


def band(rho):
    return LO if rho < 0.25 else (HI if rho > 0.75 else MID)


# solve paths (the `paths` of a case; tests/test_trust_region_branches_gpu.py runs a case on each of them)
MULTI, POLL, ONE = "multi-launch", "multi-launch, polling feed", "one-launch"
ADD1, ADD2, VCYCLE = "one-launch additive, one tile", "one-launch additive, two tiles", "V-cycle"
SYM, SYM_HOST = "symmetric storage, outer kernels", "symmetric storage, DPGO_OUTER_SYM=0"
LINEAR = "linear term"
DEVICE, BEGIN_END, MANY = "optimizeDevice", "optimizeDeviceBegin/End", "optimize_device_many"
ENTRIES = (DEVICE, BEGIN_END, MANY)
ORACLE_PRECOND = {"jacobi": "jacobi", "none": "none", "additive": "amg_additive", "multilevel": "amg"}


@dataclass(frozen=True)
class Case:
    """problem: ("random", d, linear term?) | ("data", name) | ("lattice", nx, ny) | ("grid", nx, ny, nz);
    start: ("random", seed) | ("chordal",) | ("noisy", sigma, seed)."""
    name: str
    problem: tuple
    r: int
    precond: str
    start: tuple
    radius: float  # RTR_initial_radius of the trajectory
    k: int  # the window starts in front of the trajectory's outer iteration k
    expect: tuple  # ((exit, band, decision), ...), one per outer iteration of the window
    paths: tuple
    kind: str = "window"  # "window" | "clip" | "all-rejected" | "shrink" | "give-up"
    tiny: bool = True  # accept_tiny_decrease, both sides
    tcg_iterations: int = 50
    trajectory: int = TRAJECTORY
    ks: Optional[tuple] = None  # aggregate sizes of the hierarchy, where the block's size does not give them
    then: str = ""  # all-rejected: the case (same problem, same start) solved on the same handle afterwards

    @property
    def iterations(self):
        return len(self.expect)


_PROBLEMS, _TRAJECTORIES = {}, {}


def random_problem_size(d, r):
    return 150 + 7 * r + d


def build_problem(oracle, case):
    """dict(om, n, d, Q, G) of a case (cached per problem and rank: G has the rank in its shape)."""
    from test_parity_gpu import _grid2d_measurements, _random_graph
    key = (case.problem, case.r)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    kind, G = case.problem[0], None
    if kind == "random":
        d = case.problem[1]
        n = random_problem_size(d, case.r)
        om, _, _ = _random_graph(oracle, d, n, n // 2, 20, seed=40 + n)
        if case.problem[2]:  # the multi-agent cost f = 0.5 <X Q, X> + <X, G>
            G = 0.5 * np.random.default_rng(7 + n).standard_normal((n, d + 1, case.r))
    elif kind == "data":
        om, n = oracle.read_g2o(os.path.join(DATA, case.problem[1] + ".g2o"))
    elif kind == "lattice":
        om, n = _grid2d_measurements(oracle, case.problem[1], case.problem[2], seed=4)
    elif kind == "grid":
        om, n, _ = oracle.synthetic_grid(*case.problem[1:], seed=0)
    else:
        raise ValueError(kind)
    d = om.d
    _PROBLEMS[key] = dict(om=om, n=n, d=d, Q=oracle.construct_Q(n, d, om), G=G)
    return _PROBLEMS[key]


def build_start(oracle, case):
    from test_parity_gpu import random_point
    p = build_problem(oracle, case)
    n, d, r = p["n"], p["d"], case.r
    if case.start[0] == "random":
        return random_point(oracle, n, d, r, case.start[1])
    if case.start[0] == "chordal":
        return oracle.lift(oracle.chordal_initialization(p["om"], n), r)
    if case.start[0] == "noisy":  # polar_project(lift(T) + sigma randn), T the ground truth of the synthetic grid
        _, _, T = oracle.synthetic_grid(*case.problem[1:], seed=0)
        rng = np.random.default_rng(case.start[2])
        return oracle.polar_project(oracle.lift(T, r) + case.start[1] * rng.standard_normal((n, d + 1, r)), d)
    raise ValueError(case.start)


def default_ks(oracle, case):
    """Aggregate sizes of the hierarchy the device builds for this block (asserted against the handle's on the GPU)."""
    p = build_problem(oracle, case)
    if case.ks is not None:
        return list(case.ks)
    if case.precond == "additive":
        return [-(16 if p["d"] == 3 else 20)]  # graph aggregates, four lane groups per pose (<= 256 aggregates)
    if case.precond == "multilevel":
        return oracle.amg_default_ks(p["n"], p["d"] + 1)
    return None


def oracle_problem(oracle, case, ks=None):
    p = build_problem(oracle, case)
    kw = {}
    if case.precond in ("additive", "multilevel"):
        kw["amg_k"] = ks if ks is not None else default_ks(oracle, case)
    return oracle.QuadraticProblem(p["Q"], p["G"], case.r, p["d"], precond=ORACLE_PRECOND[case.precond], **kw)


def trajectory(oracle, case, ks=None):
    """The oracle's verbose trace of the long run the case's window is cut from."""
    key = (case.problem, case.r, case.precond, case.start, case.radius, case.trajectory, case.tcg_iterations, case.tiny,
           tuple(ks) if ks is not None else None)
    if key not in _TRAJECTORIES:
        prm = oracle.ROptParameters(RTR_iterations=max(2, case.trajectory), RTR_initial_radius=case.radius, verbose=True,
                                    RTR_tCG_iterations=case.tcg_iterations)
        oo = oracle.QuadraticOptimizer(oracle_problem(oracle, case, ks), prm, accept_tiny_decrease=case.tiny,
                                       hess_recurrence=True)
        oo.optimize(build_start(oracle, case))
        _TRAJECTORIES[key] = oo.result.trace
    return _TRAJECTORIES[key]


def window_start(oracle, case, ks=None):
    """(x_k, Delta_k): where the window starts.  The single-iteration kinds start at the case's own start."""
    if case.kind in ("shrink", "give-up") or case.k == 0:
        return build_start(oracle, case), case.radius
    row = trajectory(oracle, case, ks)[case.k]
    return row["x"], row["Delta_in"]


def window_parameters(oracle, case, radius):
    it = 1 if case.kind in ("shrink", "give-up") else case.iterations
    return dict(RTR_iterations=it, RTR_initial_radius=radius, RTR_tCG_iterations=case.tcg_iterations)


def run_window(oracle, case, ks=None, tiny=None, hess_recurrence=True):
    """The oracle on the case's window: (X0, radius, optimizer after optimize(X0), Xopt)."""
    X0, radius = window_start(oracle, case, ks)
    prm = oracle.ROptParameters(verbose=True, **window_parameters(oracle, case, radius))
    oo = oracle.QuadraticOptimizer(oracle_problem(oracle, case, ks), prm, hess_recurrence=hess_recurrence,
                                   accept_tiny_decrease=case.tiny if tiny is None else tiny)
    Xo = oo.optimize(X0)
    return X0, radius, oo, Xo


def observed(oracle, trace):
    return tuple((oracle.TCG_NAMES[t["status"]], band(t["rho"]), ACC if t["accept"] else REJ) for t in trace)


# (the rho of each iteration of the window, from the oracle, is noted behind each case)
CASES = [
    Case('random-2-2-jacobi-k5', ('random', 2, False), 2, 'jacobi', ('random', 3), 1e3, 5,
         ((EXCR, LO, REJ), (EXCR, HI, ACC),),
         (MULTI, ONE)),  # rho -0.164 0.907
    Case('random-2-2-jacobi-k2', ('random', 2, False), 2, 'jacobi', ('random', 3), 1e3, 2,
         ((EXCR, LO, ACC), (EXCR, HI, ACC),),
         (MULTI, ONE)),  # rho 0.228 0.955
    Case('random-2-2-jacobi-k0', ('random', 2, False), 2, 'jacobi', ('random', 3), 1e3, 0,
         ((NEGC, LO, REJ), (EXCR, HI, ACC),),
         (MULTI, ONE)),  # rho -0.354 0.848
    Case('random-2-2-none-k1', ('random', 2, False), 2, 'none', ('random', 3), 1e3, 1,
         ((NEGC, LO, REJ), (NEGC, LO, REJ), (EXCR, MID, ACC),),
         (MULTI, ONE)),  # rho -2.210 -0.585 0.518
    Case('random-2-3-jacobi-k2', ('random', 2, False), 3, 'jacobi', ('random', 3), 1e3, 2,
         ((EXCR, LO, REJ), (EXCR, HI, ACC),),
         (MULTI, POLL, ONE)),  # rho 0.053 0.904
    Case('random-2-3-jacobi-k0', ('random', 2, False), 3, 'jacobi', ('random', 3), 1e3, 0,
         ((NEGC, LO, REJ), (EXCR, HI, ACC),),
         (MULTI, ONE)),  # rho -0.492 0.813
    Case('random-2-3-jacobi-k6', ('random', 2, False), 3, 'jacobi', ('random', 3), 1e3, 6,
         ((NEGC, LO, REJ), (EXCR, HI, ACC),),
         (MULTI, ONE)),  # rho -0.553 1.004
    Case('random-2-3-none-k1', ('random', 2, False), 3, 'none', ('random', 3), 1e3, 1,
         ((NEGC, LO, REJ), (NEGC, LO, REJ), (EXCR, MID, ACC),),
         (MULTI, ONE)),  # rho -0.259 -0.064 0.553
    Case('random-2-4-jacobi-k5', ('random', 2, False), 4, 'jacobi', ('random', 3), 1e3, 5,
         ((EXCR, LO, REJ), (EXCR, HI, ACC),),
         (MULTI, ONE)),  # rho -0.087 0.998
    Case('random-2-4-jacobi-k2', ('random', 2, False), 4, 'jacobi', ('random', 3), 1e3, 2,
         ((EXCR, LO, ACC), (EXCR, HI, ACC),),
         (MULTI, ONE)),  # rho 0.112 1.025
    Case('random-2-4-none-k1', ('random', 2, False), 4, 'none', ('random', 3), 1e3, 1,
         ((NEGC, LO, REJ), (NEGC, LO, REJ), (EXCR, MID, ACC),),
         (MULTI, ONE)),  # rho -0.217 -0.096 0.474
    Case('random-2-5-jacobi-k4', ('random', 2, False), 5, 'jacobi', ('random', 3), 1e3, 4,
         ((NEGC, LO, REJ), (EXCR, HI, ACC),),
         (MULTI, ONE)),  # rho -0.349 0.951
    Case('random-2-5-none-k1', ('random', 2, False), 5, 'none', ('random', 3), 1e3, 1,
         ((NEGC, LO, REJ), (NEGC, LO, REJ), (EXCR, MID, ACC),),
         (MULTI, ONE)),  # rho -0.141 -0.028 0.420
    Case('random-3-3-jacobi-k1', ('random', 3, False), 3, 'jacobi', ('random', 3), 1e3, 1,
         ((EXCR, MID, ACC), (NEGC, MID, ACC), (NEGC, LO, REJ),),
         (MULTI, ONE)),  # rho 0.695 0.286 -0.106
    Case('random-3-3-jacobi-k3', ('random', 3, False), 3, 'jacobi', ('random', 3), 1e3, 3,
         ((NEGC, LO, REJ), (EXCR, HI, ACC),),
         (MULTI, ONE)),  # rho -0.106 0.879
    Case('random-3-3-none-k1', ('random', 3, False), 3, 'none', ('random', 3), 1e3, 1,
         ((NEGC, LO, REJ), (NEGC, LO, REJ), (EXCR, MID, ACC),),
         (MULTI, ONE)),  # rho -0.611 -0.225 0.681
    Case('random-3-4-jacobi-k0', ('random', 3, False), 4, 'jacobi', ('random', 3), 1e3, 0,
         ((EXCR, LO, REJ), (EXCR, HI, ACC),),
         (MULTI, ONE)),  # rho -0.995 0.848
    Case('random-3-4-jacobi-k2', ('random', 3, False), 4, 'jacobi', ('random', 3), 1e3, 2,
         ((NEGC, LO, REJ), (EXCR, HI, ACC),),
         (MULTI, ONE)),  # rho 0.060 0.964
    Case('random-3-4-none-k1', ('random', 3, False), 4, 'none', ('random', 3), 1e3, 1,
         ((NEGC, LO, REJ), (NEGC, LO, REJ), (EXCR, MID, ACC),),
         (MULTI, ONE)),  # rho -0.512 -0.070 0.709
    Case('random-3-5-jacobi-k3', ('random', 3, False), 5, 'jacobi', ('random', 3), 1e3, 3,
         ((NEGC, LO, REJ), (EXCR, HI, ACC),),
         (MULTI, POLL, ONE) + ENTRIES),  # rho 0.020 0.842
    Case('random-3-5-jacobi-k6', ('random', 3, False), 5, 'jacobi', ('random', 3), 1e3, 6,
         ((EXCR, LO, REJ), (EXCR, HI, ACC),),
         (MULTI, ONE)),  # rho -0.082 0.904
    Case('random-3-5-none-k1', ('random', 3, False), 5, 'none', ('random', 3), 1e3, 1,
         ((NEGC, LO, REJ), (NEGC, LO, REJ), (EXCR, MID, ACC),),
         (MULTI, ONE)),  # rho -0.139 -0.035 0.380
    Case('random-3-6-jacobi-k3', ('random', 3, False), 6, 'jacobi', ('random', 3), 1e3, 3,
         ((NEGC, LO, REJ), (EXCR, HI, ACC),),
         (MULTI, ONE)),  # rho 0.072 0.846
    Case('random-3-6-jacobi-k6', ('random', 3, False), 6, 'jacobi', ('random', 3), 1e3, 6,
         ((EXCR, LO, ACC), (EXCR, HI, ACC),),
         (MULTI, ONE)),  # rho 0.215 1.015
    Case('random-3-6-none-k1', ('random', 3, False), 6, 'none', ('random', 3), 1e3, 1,
         ((NEGC, LO, REJ), (NEGC, LO, REJ), (EXCR, MID, ACC),),
         (MULTI, ONE)),  # rho -0.125 -0.043 0.347
    Case('random-3-5-none-k4', ('random', 3, False), 5, 'none', ('random', 3), 1e3, 4,
         ((NEGC, LO, ACC), (EXCR, MID, ACC),),
         (MULTI, ONE)),  # rho 0.190 0.535
    # (tCG left through negative curvature and rho > 0.75: the radius doubles as after EXCREGION)
    Case('random-3-4-jacobi-seed7-k1', ('random', 3, False), 4, 'jacobi', ('random', 7), 1e3, 1,
         ((NEGC, HI, ACC), (EXCR, LO, ACC),),
         (MULTI, ONE)),  # rho 0.853 0.124
    Case('random-3-5-jacobi-seed5-k3', ('random', 3, False), 5, 'jacobi', ('random', 5), 1e3, 3,
         ((NEGC, HI, ACC), (EXCR, HI, ACC),),
         (MULTI, ONE)),  # rho 0.823 0.968
    Case('random-2-2-none-seed4-k3', ('random', 2, False), 2, 'none', ('random', 4), 100.0, 3,
         ((NEGC, HI, ACC), (EXCR, MID, ACC),),
         (MULTI, ONE)),  # rho 0.777 0.575
    Case('random-3-5-none-seed1-k4', ('random', 3, False), 5, 'none', ('random', 1), 100.0, 4,
         ((NEGC, HI, ACC), (EXCR, MID, ACC),),
         (MULTI, ONE)),  # rho 0.873 0.558
    Case('linear-2-3-jacobi-k2', ('random', 2, True), 3, 'jacobi', ('random', 3), 1e3, 2,
         ((EXCR, LO, REJ), (EXCR, HI, ACC),),
         (LINEAR,)),  # rho 0.052 0.904
    Case('linear-2-3-jacobi-k6', ('random', 2, True), 3, 'jacobi', ('random', 3), 1e3, 6,
         ((NEGC, LO, REJ), (EXCR, HI, ACC),),
         (LINEAR,)),  # rho -0.606 1.002
    Case('linear-3-5-jacobi-k3', ('random', 3, True), 5, 'jacobi', ('random', 3), 1e3, 3,
         ((NEGC, LO, REJ), (EXCR, HI, ACC),),
         (LINEAR,)),  # rho 0.028 0.847
    Case('linear-3-5-none-k1', ('random', 3, True), 5, 'none', ('random', 3), 1e3, 1,
         ((NEGC, LO, REJ), (NEGC, LO, REJ), (EXCR, MID, ACC),),
         (LINEAR,)),  # rho -0.139 -0.035 0.380
    Case('clip-sphere2500-5', ('data', 'sphere2500'), 5, 'jacobi', ('random', 3), 100.0, 0,
         ((EXCR, HI, ACC), (EXCR, HI, ACC), (EXCR, HI, ACC), (EXCR, HI, ACC),),
         (MULTI, ONE), kind='clip'),  # rho 1.000 0.998 0.980 0.930
    Case('clip-kitti_00-3', ('data', 'kitti_00'), 3, 'jacobi', ('random', 3), 100.0, 0,
         ((EXCR, HI, ACC), (EXCR, HI, ACC), (EXCR, HI, ACC), (EXCR, HI, ACC),),
         (MULTI, ONE), kind='clip'),  # rho 1.000 1.000 1.000 1.000
    Case('all-rejected-2-3-jacobi', ('random', 2, False), 3, 'jacobi', ('random', 3), 1e6, 0,
         ((NEGC, LO, REJ), (NEGC, LO, REJ),),
         (MULTI, ONE) + ENTRIES, kind='all-rejected', then='random-2-3-jacobi-k0'),  # rho -1.878 -1.872
    Case('all-rejected-3-5-none', ('random', 3, False), 5, 'none', ('random', 3), 1e6, 0,
         ((NEGC, LO, REJ), (NEGC, LO, REJ),),
         (MULTI, ONE) + ENTRIES, kind='all-rejected', then='random-3-5-none-k1'),  # rho -0.152 -0.152
    Case('all-rejected-3-4-jacobi', ('random', 3, False), 4, 'jacobi', ('random', 3), 1e6, 0,
         ((NEGC, LO, REJ), (NEGC, LO, REJ),),
         (MULTI, ONE) + ENTRIES, kind='all-rejected', then='random-3-4-jacobi-k0'),  # rho -68.177 -68.173
    Case('shrink-2-3-jacobi', ('random', 2, False), 3, 'jacobi', ('random', 3), 1e4, 0,
         ((NEGC, LO, REJ), (NEGC, LO, REJ), (NEGC, LO, REJ), (EXCR, HI, ACC),),
         (MULTI,), kind='shrink'),  # rho -1.689 -1.191 -0.022 0.921
    Case('shrink-3-5-jacobi', ('random', 3, False), 5, 'jacobi', ('random', 3), 1e4, 0,
         ((NEGC, LO, REJ), (NEGC, LO, REJ), (NEGC, LO, ACC),),
         (MULTI,), kind='shrink'),  # rho -1.295 -0.905 0.115
    Case('shrink-2-5-none', ('random', 2, False), 5, 'none', ('random', 3), 1e4, 0,
         ((NEGC, LO, REJ), (NEGC, LO, REJ), (NEGC, LO, REJ), (NEGC, LO, REJ), (EXCR, LO, ACC),),
         (MULTI,), kind='shrink'),  # rho -0.146 -0.146 -0.146 -0.131 0.136
    Case('give-up-2-3-jacobi', ('random', 2, False), 3, 'jacobi', ('random', 3), 1e12, 0,
         ((NEGC, LO, REJ),) * 12,
         (MULTI,), kind='give-up'),  # rho -1.879 -1.879 -1.879 -1.879 -1.879 -1.879 -1.879 -1.879 -1.879 -1.879 -1.877 -1.871
    Case('give-up-3-5-none', ('random', 3, False), 5, 'none', ('random', 3), 1e12, 0,
         ((NEGC, LO, REJ),) * 12,
         (MULTI,), kind='give-up'),  # rho -0.152 -0.152 -0.152 -0.152 -0.152 -0.152 -0.152 -0.152 -0.152 -0.152 -0.152 -0.152
    Case('lattice-additive-1000-k0', ('lattice', 40, 30), 3, 'additive', ('chordal',), 1e3, 0,
         ((NEGC, LO, REJ), (EXCR, MID, ACC),),
         (ADD1,), trajectory=10),  # rho -2.253 0.505
    Case('lattice-additive-1000-k4', ('lattice', 40, 30), 3, 'additive', ('chordal',), 1e3, 4,
         ((NEGC, LO, REJ), (EXCR, HI, ACC),),
         (ADD1,), trajectory=10),  # rho -0.048 1.009
    Case('lattice-additive-100-k4', ('lattice', 40, 30), 3, 'additive', ('chordal',), 100.0, 4,
         ((EXCR, LO, ACC), (EXCR, HI, ACC),),
         (ADD1,), trajectory=10),  # rho 0.197 1.013
    Case('sphere2500-additive-k0', ('data', 'sphere2500'), 5, 'additive', ('random', 1), 1e4, 0,
         ((NEGC, LO, REJ), (NEGC, LO, REJ), (EXCR, HI, ACC),),
         (ADD1,)),  # rho -1.158 -0.560 0.872
    Case('sphere2500-additive-k3', ('data', 'sphere2500'), 5, 'additive', ('random', 1), 1e4, 3,
         ((NEGC, LO, REJ), (NEGC, MID, ACC),),
         (ADD1,)),  # rho 0.064 0.616
    Case('lattice-multilevel-1000-k0', ('lattice', 40, 30), 3, 'multilevel', ('chordal',), 1e3, 0,
         ((NEGC, LO, REJ), (EXCR, MID, ACC),),
         (VCYCLE,), trajectory=10),  # rho -1.938 0.469
    Case('lattice-multilevel-100-k4', ('lattice', 40, 30), 3, 'multilevel', ('chordal',), 100.0, 4,
         ((EXCR, LO, REJ), (EXCR, HI, ACC),),
         (VCYCLE,), trajectory=10),  # rho 0.048 1.013
    Case('lattice-multilevel-100-k6', ('lattice', 40, 30), 3, 'multilevel', ('chordal',), 100.0, 6,
         ((EXCR, LO, REJ), (EXCR, HI, ACC),),
         (VCYCLE,), trajectory=10),  # rho -0.072 0.979
    Case('sphere2500-multilevel-k0', ('data', 'sphere2500'), 5, 'multilevel', ('random', 1), 1e4, 0,
         ((NEGC, LO, REJ), (NEGC, LO, REJ),),
         (VCYCLE,)),  # rho -0.564 0.006
    Case('grid-40x40x25-symmetric', ('grid', 40, 40, 25), 5, 'jacobi', ('noisy', 0.7, 5), 1e4, 0,
         ((NEGC, MID, ACC), (EXCR, LO, REJ), (EXCR, HI, ACC),),
         (SYM, SYM_HOST)),  # rho 0.566 -0.008 0.971
    Case('grid-30x30x20-two-tile', ('grid', 30, 30, 20), 5, 'additive', ('noisy', 0.7, 5), 1e4, 2,
         ((NEGC, LO, REJ), (EXCR, HI, ACC),),
         (ADD2,), ks=(-79, -118)),  # rho -0.344 0.986
]


def by_name(name):
    return next(c for c in CASES if c.name == name)
