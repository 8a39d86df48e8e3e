"""Certificate of global optimality and the Riemannian staircase (C ABI dpgo_problem_certify*).

  QuadraticProblem.certify(X)            lambda_min of C(X) = Q - Lambda(X) on the complement of the known null space, by a
                                         preconditioned block LOBPCG on the device -> CertificateResult (+ witness)
  QuadraticProblem.certificateApply(X, V)  V C(X) (tests)
  certify_team(agents)                   the same for the iterate of a TEAM of DeviceAgents on one device, from the agents'
                                         own blocks (Q_aa, the G coupling): no central copy of the problem is built
  solveCertifiedPGO(measurements)        SE-Sync's staircase on one handle per rank: solve, certify, escape to rank r + 1
                                         along the witness while the iterate is a saddle; rounds the certified iterate
  evaluate_team(agents)                  f and |rgrad f| of the team's iterate in one launch, without an exchange
  escape_team(agents, witness, ...)      the team's staircase step: agents at rank r + 1 at the lifted, retracted iterate
  solveCertifiedDistributedPGO(...)      the staircase for a team: RBCD sweeps, certify_team, escape_team

Certification is defined for a problem WITHOUT a linear term G (the global or central problem: no shared loop closures, no
priors).  CERTIFIED is numerical (the eigen-solver's smallest Ritz value on the complement is >= -eta scale with a small
residual), not a lower-bound proof; NOT_CERTIFIED is a proof up to rounding (the witness has w^T C w < -eta scale).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import lib as L
from .measurements import RelativeSEMeasurements

PRECONDS = {"none": L.PRECOND_NONE, "jacobi": L.PRECOND_BLOCK_JACOBI, "multilevel": L.PRECOND_MULTILEVEL,
            "auto": L.PRECOND_AUTO, "additive": L.PRECOND_ADDITIVE}


@dataclass
class CertificateResult:
    """dpgo_certify_result; status CERTIFIED | NOT_CERTIFIED | NOT_CONVERGED; witness: (n, d+1) unit vector or None."""
    status: str
    lambda_min: float
    residual: float
    gradnorm: float
    scale: float
    iterations: int
    products: int
    deflated: int
    deflation_residual: float
    elapsedMs: float
    witness: Optional[np.ndarray] = None
    symmetry_defect: Optional[float] = None  # certify_team: the probe of the agents' pieces (None for one handle)

    @staticmethod
    def from_c(c: L.CertifyResultC, witness=None) -> "CertificateResult":
        return CertificateResult(L.CERT_STATUS[c.status], c.lambda_min, c.residual, c.gradnorm, c.scale, c.iterations,
                                 c.products, c.deflated, c.deflation_residual, c.elapsedMs, witness)


def certify_params(eta: Optional[float] = None, tol_rel: Optional[float] = None, max_iterations: Optional[int] = None,
                   precond: Optional[str] = None, precond_shift: Optional[float] = None,
                   seed: Optional[int] = None) -> L.CertifyParamsC:
    """dpgo_certify_params: the library's defaults (dpgo_certify_params_default) with the given fields replaced."""
    c = L.CertifyParamsC()
    L.load().dpgo_certify_params_default(C.byref(c))
    if eta is not None:
        c.eta = float(eta)
    if tol_rel is not None:
        c.tol_rel = float(tol_rel)
    if max_iterations is not None:
        c.max_iterations = int(max_iterations)
    if precond is not None:
        if precond not in PRECONDS:
            raise ValueError("unknown preconditioner %r (one of %s)" % (precond, sorted(PRECONDS)))
        c.precond = PRECONDS[precond]
    if precond_shift is not None:
        c.precond_shift = float(precond_shift)
    if seed is not None:
        c.seed = int(seed)
    if not (c.eta >= 0 and c.tol_rel > 0 and c.max_iterations >= 1 and c.precond_shift >= 0):
        raise ValueError("bad certification parameters (eta >= 0, tol_rel > 0, max_iterations >= 1, precond_shift >= 0)")
    return c


def check_certifiable(pose_graph, X=None) -> None:
    """Host-side checks made before any device work: no linear term G (shared loop closures, priors), a compiled (d, r),
    X of shape (r, (d+1) n)."""
    r, d, n = pose_graph.r(), pose_graph.d(), pose_graph.n()
    if len(pose_graph.sharedLoopClosures()) > 0 or len(pose_graph.priors_) > 0:
        raise ValueError("certification is defined for a problem without a linear term G (no shared loop closures, "
                         "no priors): certify the assembled global problem on one central handle")
    if not L.load().dpgo_supported(d, r):
        raise ValueError("(d, r) = (%d, %d) has no compiled kernels" % (d, r))
    if X is not None:
        X = np.asarray(X)
        if X.shape != (r, (d + 1) * n):
            raise ValueError("X has shape %s, expected (%d, %d)" % (X.shape, r, (d + 1) * n))


def certify(problem, X, witness: bool = True, **params) -> CertificateResult:
    """QuadraticProblem.certify: certificate of the rank-r iterate X (host matrix r x (d+1)n)."""
    check_certifiable(problem.pose_graph_, X)
    cp = certify_params(**params)
    problem.refresh()
    Xc = problem._in(X, "X")
    n, d = problem.num_poses(), problem.dimension()
    w = np.empty(n * (d + 1)) if witness else None
    cr = L.CertifyResultC()
    L.check(problem._lib.dpgo_problem_certify(problem._h, L.ptr(Xc), C.byref(cp), C.byref(cr),
                                              L.ptr(w) if w is not None else None))
    return CertificateResult.from_c(cr, w.reshape(n, d + 1) if w is not None else None)


def certificate_apply(problem, X, V) -> np.ndarray:
    """QuadraticProblem.certificateApply: V C(X) for host matrices X, V (r x (d+1)n)."""
    check_certifiable(problem.pose_graph_, X)
    check_certifiable(problem.pose_graph_, V)
    problem.refresh()
    Xc, Vc, o = problem._in(X, "X"), problem._in(V, "V"), problem._out()
    L.check(problem._lib.dpgo_problem_certificate_apply(problem._h, L.ptr(Xc), L.ptr(Vc), L.ptr(o)))
    return o


# ---------------------------------------------------------------- a team of agents on one device
def team_layout(agents):
    """(firsts, N, nbr_pose) of a team (C ABI dpgo_team_member): agent a owns tiles [firsts[a], firsts[a] + n_a) of the
    team vector in its internal pose order; nbr_pose[a][k] = team tile of column slot k of its G coupling
    (ExchangePlan.slots[a][k] = (robot, frame), frames in the robots' internal numbering)."""
    ids = [int(ag.id) for ag in agents]
    if ids != list(range(len(agents))) or len(agents) != agents[0].plan.num_agents:
        raise ValueError("a team is every agent of the plan, in id order (got ids %s)" % ids)
    return team_nbr_pose(agents[0].plan, [int(ag.n) for ag in agents])


def team_nbr_pose(plan, ns):
    """team_layout from an ExchangePlan and the agents' pose counts (host only).  Kept with the plan, which is static: the
    sweep loop of the staircase asks for it at every evaluation."""
    key = tuple(int(v) for v in ns)
    cache = plan.__dict__.setdefault("_team_layouts", {})
    if key not in cache:
        firsts = [int(v) for v in np.concatenate([[0], np.cumsum(ns)[:-1]])]
        nbr = [np.array([firsts[rob] + fr for rob, fr in plan.slots[a]], dtype=np.int32) for a in range(len(ns))]
        cache[key] = (firsts, int(sum(ns)), nbr)
    firsts, N, nbr = cache[key]
    return list(firsts), N, nbr


def _team_members(agents, firsts, nbr):
    arr = (L.TeamMemberC * len(agents))()
    for a, ag in enumerate(agents):
        ag.problem.refresh()
        arr[a].h, arr[a].first = ag.problem._h, firsts[a]
        arr[a].nbr_pose = nbr[a].ctypes.data if len(nbr[a]) else None
    return arr


def _team_list(agents):
    agents = [agents[k] for k in sorted(agents)] if isinstance(agents, dict) else list(agents)
    if not agents:
        raise ValueError("an empty team")
    for ag in agents:
        if len(ag.pg.priors_) > 0:
            raise ValueError("certify_team: agent %d has priors (a constant term in G): out of scope" % ag.id)
    return agents


def certify_team(agents, witness: bool = True, **params) -> CertificateResult:
    """Certificate of the team's current iterate (the agents' X, concatenated device to device) from the agents' own
    handles: dpgo_team_certify_device.  agents: every DeviceAgent of one ExchangePlan, on one device (a list in id order
    or {id: agent}).  The witness comes back in the caller's global pose order, (N, d+1).  The call refreshes every
    agent's linear term G from the team's X, as an exchange of the certified iterate would.  Raises DpgoError (ERR_STATE)
    when the agents hold different weights or activity for a shared edge (symmetry_defect, include/dpgo_hip.h)."""
    agents = _team_list(agents)
    torch = agents[0].torch
    cp = certify_params(**params)
    firsts, N, nbr = team_layout(agents)
    d = agents[0].d
    X = torch.cat([ag.X for ag in agents]).contiguous()
    w = torch.empty(N * (d + 1), dtype=torch.float64, device=X.device) if witness else None
    torch.cuda.synchronize(X.device)
    cr = L.TeamCertifyResultC()
    L.check(L.load().dpgo_team_certify_device(_team_members(agents, firsts, nbr), len(agents), L.ptr(X), C.byref(cp),
                                              C.byref(cr), L.ptr(w) if w is not None else None))
    wh = None
    if w is not None:
        wt = w.cpu().numpy().reshape(N, d + 1)
        wh = np.concatenate([ag.in_caller_order(wt[f:f + ag.n]) for ag, f in zip(agents, firsts)])
    res = CertificateResult.from_c(cr.cert, wh)
    res.symmetry_defect = cr.symmetry_defect
    return res


def team_certificate_apply(agents, V_tiles, gram: bool = False):
    """V C(X) at the team's current iterate for team tiles V [N, d+1, r] in team order (host array; tests):
    dpgo_team_certificate_apply_device.  gram: also the r x r block V (CV)^T the kernel sums on the way."""
    agents = _team_list(agents)
    torch = agents[0].torch
    firsts, N, nbr = team_layout(agents)
    X = torch.cat([ag.X for ag in agents]).contiguous()
    V = torch.as_tensor(np.ascontiguousarray(V_tiles), dtype=torch.float64, device=X.device)
    if tuple(V.shape) != tuple(X.shape):
        raise ValueError("V has shape %s, expected %s" % (tuple(V.shape), tuple(X.shape)))
    CV = torch.empty_like(V)
    torch.cuda.synchronize(X.device)
    r = agents[0].r
    vcv = np.empty((r, r)) if gram else None
    L.check(L.load().dpgo_team_certificate_apply_gram_device(_team_members(agents, firsts, nbr), len(agents), L.ptr(X),
                                                             L.ptr(V), L.ptr(CV), L.ptr(vcv)))
    out = CV.cpu().numpy()
    return (out, vcv) if gram else out


def evaluate_team(agents, gradient: bool = False):
    """(f, |rgrad f|) of the team's current iterate from the agents' own blocks in one launch (dpgo_team_eval_device): no
    exchange, the agents' G and neighbour buffers are not touched.  gradient: also the Riemannian gradient tiles
    [N, d+1, r] in team order (host array)."""
    agents = _team_list(agents)
    torch = agents[0].torch
    firsts, _N, nbr = team_layout(agents)
    X = torch.cat([ag.X for ag in agents]).contiguous()
    RG = torch.empty_like(X) if gradient else None
    torch.cuda.synchronize(X.device)
    f, gn = C.c_double(0.0), C.c_double(0.0)
    L.check(L.load().dpgo_team_eval_device(_team_members(agents, firsts, nbr), len(agents), L.ptr(X), C.byref(f),
                                           C.byref(gn), L.ptr(RG)))
    return (f.value, gn.value, RG.cpu().numpy()) if gradient else (f.value, gn.value)


def _in_robust_mode(ag) -> bool:
    return getattr(ag.problem, "reweightable_index", None) is not None


def escape_team(agents, witness, graphs_next, grad_tol: float, params=None):
    """The staircase step of a team: (agents at rank r + 1, their ExchangePlan, escape record).

    agents: the team at rank r (certify_team's); witness: (N, d+1) in the caller's pose order, as certify_team returns it;
    graphs_next: the same robots' PoseGraphs at rank r + 1 (build_pose_graphs of the same measurements and partition);
    params: the ROptParameters of the new agents.  dpgo_team_escape_device picks the step on the concatenated device
    iterate; every new agent is handed its slice of the lifted, retracted team vector.  Robust (GNC) weights are not
    carried across a lift: a team with an agent in robust mode is refused."""
    from .agent import DeviceAgent, ExchangePlan
    agents = _team_list(agents)
    for ag in agents:
        if _in_robust_mode(ag):
            raise ValueError("escape_team: agent %d is in robust mode; its weights are not carried across a lift" % ag.id)
    torch = agents[0].torch
    d, r = agents[0].d, agents[0].r
    firsts, N, _nbr = team_layout(agents)
    if len(graphs_next) != len(agents) or any(g.r() != r + 1 or g.n() != ag.n for g, ag in zip(graphs_next, agents)):
        raise ValueError("escape_team: graphs_next are the same robots' pose graphs at rank %d" % (r + 1))
    w = np.asarray(witness, dtype=np.float64).reshape(N, d + 1)
    wt = np.empty_like(w)  # caller's pose order -> team order (the inverse of certify_team's in_caller_order)
    for ag, f in zip(agents, firsts):
        if ag.pose_order is None:
            wt[f:f + ag.n] = w[f:f + ag.n]
        else:
            wt[f:f + ag.n][ag.pose_order] = w[f:f + ag.n]
    plan = ExchangePlan(graphs_next)
    dev = agents[0].device
    nxt = [DeviceAgent(graphs_next, plan, a, np.zeros((ag.n, d + 1, r + 1)), params, device=dev.index or 0)
           for a, ag in enumerate(agents)]
    # (the slices are handed over in the agents' internal pose order, which the graphs of one partition share)
    firsts_n, _N, nbr_n = team_layout(nxt)
    if firsts_n != firsts or any((a.pose_order is None) != (b.pose_order is None) or (
            a.pose_order is not None and not np.array_equal(a.pose_order, b.pose_order)) for a, b in zip(agents, nxt)):
        raise ValueError("escape_team: graphs_next number the poses differently from the team's graphs")
    X = torch.cat([ag.X for ag in agents]).contiguous()
    w_dev = torch.from_numpy(np.ascontiguousarray(wt.reshape(-1))).to(dev)
    Xn = torch.empty((N, d + 1, r + 1), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    out = L.TeamEscapeResultC()
    L.check(L.load().dpgo_team_escape_device(_team_members(nxt, firsts, nbr_n), len(nxt), r, L.ptr(X), L.ptr(w_dev),
                                             float(grad_tol), L.ptr(Xn), C.byref(out)))
    for ng, f in zip(nxt, firsts):
        ng.X.copy_(Xn[f:f + ng.n])
    record = dict(rank=r, alpha=out.alpha, trials=out.trials, f_before=out.f_before, f_after=out.f_after,
                  gradnorm_after=out.gradnorm_after)
    return nxt, plan, record


@dataclass
class CertifiedPGOResult:
    """Outcome of solveCertifiedPGO.  status: CERTIFIED | RANK_LIMIT (a saddle at the largest compiled / allowed rank) |
    NOT_CONVERGED (the eigen-solver's budget ended).  f: f(X) of the final rank-r iterate -- a lower bound on the PGO optimum
    when CERTIFIED; gap = f(rounded) - f(X) >= 0: an upper bound on the suboptimality of the rounded trajectory."""
    trajectory: np.ndarray  # d x (d+1)n, pose 0 at the origin (round_trajectory)
    rank: int
    status: str
    f: float
    f_rounded: float
    gap: float
    certificate: CertificateResult
    X: np.ndarray  # the final rank-r iterate, r x (d+1)n
    escapes: List[dict] = field(default_factory=list)  # one entry per escape: rank, lambda_min, alpha, f before / after


def _poses_to_matrix(T: np.ndarray, r: int) -> np.ndarray:
    """tiles [n, d+1, d] -> r x (d+1)n, the rotation block lifted by [I_d; 0]."""
    n, b, d = T.shape
    X = np.zeros((r, n * b), order="F")
    X[:d, :] = T.reshape(n * b, d).T
    return X


def solveCertifiedPGO(measurements: RelativeSEMeasurements, r0: Optional[int] = None, r_max: Optional[int] = None,
                      params: Optional[dict] = None, X0=None, ropt=None, grad_tol: float = 1e-9, max_solves: int = 50,
                      device: int = 0) -> CertifiedPGOResult:
    """SE-Sync's Riemannian staircase for one robot's pose graph (measurements of robot 0 only).

    r0: first rank (default d); r_max: last rank (default: the largest compiled one); params: certify() keyword arguments;
    X0: initial poses as tiles [n, d+1, d] or an r0 x (d+1)n matrix (default: chordal initialisation); ropt: the
    ROptParameters of the solves at every rank (default: RTR to |rgrad| <= grad_tol, repeated up to max_solves times)."""
    from .solver import PoseGraph, QuadraticOptimizer, QuadraticProblem, ROptParameters
    from .trajectory import round_trajectory

    d = measurements.d
    n = int(max(int(np.max(measurements.p1)), int(np.max(measurements.p2)))) + 1 if len(measurements) else 0
    r0 = d if r0 is None else int(r0)
    lib = L.load()
    if r0 < d or not lib.dpgo_supported(d, r0):
        raise ValueError("r0 = %d: need d <= r0 and a compiled (d, r0)" % r0)
    if r_max is None:
        r_max = r0
        while lib.dpgo_supported(d, r_max + 1):
            r_max += 1
    if np.any(measurements.r1 != measurements.r2):
        raise ValueError("solveCertifiedPGO takes the measurements of one pose graph (no inter-robot edges)")
    params = dict(params or {})
    if ropt is None:
        ropt = ROptParameters(gradnorm_tol=grad_tol, RTR_iterations=50, RTR_tCG_iterations=100)
    if X0 is None:
        from .initialization import chordal_initialization
        X = _poses_to_matrix(chordal_initialization(measurements, n, device=device), r0)
    else:
        X0 = np.asarray(X0, dtype=np.float64)
        X = _poses_to_matrix(X0, r0) if X0.ndim == 3 else np.asfortranarray(X0)

    import torch
    r = r0
    escapes: List[dict] = []
    while True:
        pg = PoseGraph(0, r, d)
        pg.setMeasurements(measurements)
        problem = QuadraticProblem(pg, device=device)
        opt = QuadraticOptimizer(problem, ropt)
        for _ in range(max_solves):
            X = opt.optimize(X)
            if opt.getOptResult().gradNormOpt <= ropt.gradnorm_tol:
                break
        cert = problem.certify(X, **params)
        if cert.status == "CERTIFIED":
            status = "CERTIFIED"
            break
        if cert.status == "NOT_CONVERGED":
            status = "NOT_CONVERGED"
            break
        if r + 1 > r_max or not lib.dpgo_supported(d, r + 1):
            status = "RANK_LIMIT"
            break
        # escape the saddle: rank r + 1 along e_{r+1} w^T
        pg_next = PoseGraph(0, r + 1, d)
        pg_next.setMeasurements(measurements)
        problem_next = QuadraticProblem(pg_next, device=device)
        dev = torch.device("cuda", device)
        X_dev = torch.from_numpy(np.ascontiguousarray(np.asfortranarray(X).T)).to(dev)
        w_dev = torch.from_numpy(np.ascontiguousarray(cert.witness.reshape(-1))).to(dev)
        Xn_dev = torch.empty((n * (d + 1), r + 1), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        alpha = C.c_double(0.0)
        L.check(lib.dpgo_certify_escape_device(problem_next._h, r, L.ptr(X_dev), L.ptr(w_dev), float(ropt.gradnorm_tol),
                                               L.ptr(Xn_dev), C.byref(alpha)))
        f_before = problem.f(X)
        X = np.asfortranarray(Xn_dev.cpu().numpy().T)
        escapes.append(dict(rank=r, lambda_min=cert.lambda_min, gradnorm=cert.gradnorm, alpha=alpha.value,
                            f_before=f_before, f_after=problem_next.f(X)))
        r += 1
    f = problem.f(X)
    T = round_trajectory(X, r, d, device=device)
    Xr = np.zeros((r, T.shape[1]), order="F")
    Xr[:d, :] = T
    f_rounded = problem.f(Xr)
    return CertifiedPGOResult(T, r, status, f, f_rounded, f_rounded - f, cert, X, escapes)


@dataclass
class DistributedCertifiedPGOResult(CertifiedPGOResult):
    """Outcome of solveCertifiedDistributedPGO: CertifiedPGOResult (trajectory and X in the caller's global pose order, the
    frame of robot 0's first pose) and the RBCD sweeps spent at every rank.  status: CERTIFIED | RANK_LIMIT | NOT_CONVERGED,
    or NOT_CONVERGED_SWEEPS: the sweeps at some rank neither brought the team's |rgrad| to grad_tol within max_sweeps nor
    moved the team to a point of rest; the iterate was not certified (certificate: the previous rank's, or None)."""
    sweeps: List[int] = field(default_factory=list)


def solveCertifiedDistributedPGO(measurements: RelativeSEMeasurements, num_poses: int, num_robots: int,
                                 r0: Optional[int] = None, r_max: Optional[int] = None, X0=None,
                                 params: Optional[dict] = None, ropt=None, grad_tol: float = 2e-6, max_sweeps: int = 2000,
                                 device: int = 0) -> DistributedCertifiedPGOResult:
    """The Riemannian staircase for a team of robots on one device: RBCD sweeps at rank r until the team's |rgrad| (one
    launch, RBCDCluster.team_cost_and_gradnorm) is at most grad_tol, certify_team, and while the iterate is a saddle
    escape_team to rank r + 1 along the witness.  No central copy of the problem is built at any point.

    measurements: the global pose graph (robot ids 0), partitioned into num_robots contiguous blocks (build_pose_graphs);
    r0: first rank (default d); r_max: last rank (default: the largest compiled one); X0: tiles [n, d+1, d] or [n, d+1, r0]
    or an r0 x (d+1)n matrix in global pose order (default: chordal initialisation lifted to r0); params: certify_team's
    keyword arguments; max_sweeps: per rank.  The sweeps at a rank also end when the team has come to rest: two
    evaluations five sweeps apart give the same bits of f and |rgrad| (every local solve stops at its own gradnorm_tol, or
    at the precision of its own cost: smallGrid3D in 5 robots rests at |rgrad| = 5e-5 with f converged to the last bit).  A
    team that moved before it came to rest is certified where it rests; one that never moved from where the rank began
    (every step rejected), or that is still moving after max_sweeps, ends the run with NOT_CONVERGED_SWEEPS.  A NOT_CERTIFIED verdict whose returned pair has no negative curvature (the eigen-solver
    ended on another pair: a tol_rel far below what the iterate's own |rgrad| supports) gives no witness: NOT_CONVERGED.

    ropt, the agents' local-solve parameters, defaults to ROptParameters(gradnorm_tol=1e-6, RTR_iterations=10,
    RTR_initial_radius=1.0), NOT to ROptParameters(): with the reference's RTR_initial_radius = 100 and RTR_iterations = 3
    a team never leaves an escaped point.  Measured with the NumPy oracle on the 16-pose identity ring from the winding-1
    saddle (2 and 4 robots, d = 2 and 3): tCG runs to the boundary of the radius-100 region, the step is rejected three
    times, every optimize call starts from radius 100 again, and over 1000 sweeps 2f stays 4.8475925434396405; with the
    defaults here the team reaches the next saddle in 25-50 sweeps and f ~ 1e-12 within 50 more."""
    from .agent import DeviceAgent, ExchangePlan, RBCDCluster, build_pose_graphs
    from .solver import ROptParameters
    from .synthetic import lift_tiles

    d, n = measurements.d, int(num_poses)
    r0 = d if r0 is None else int(r0)
    lib = L.load()
    if r0 < d or not lib.dpgo_supported(d, r0):
        raise ValueError("r0 = %d: need d <= r0 and a compiled (d, r0)" % r0)
    if r_max is None:
        r_max = r0
        while lib.dpgo_supported(d, r_max + 1):
            r_max += 1
    params = dict(params or {})
    if ropt is None:
        ropt = ROptParameters(gradnorm_tol=1e-6, RTR_iterations=10, RTR_initial_radius=1.0)
    if X0 is None:
        from .initialization import chordal_initialization
        Xt = lift_tiles(chordal_initialization(measurements, n, device=device), r0)
    else:
        X0 = np.asarray(X0, dtype=np.float64)
        if X0.ndim == 2:  # r0 x (d+1)n
            X0 = np.ascontiguousarray(np.asfortranarray(X0).T).reshape(n, d + 1, X0.shape[0])
        Xt = lift_tiles(X0, r0) if X0.shape[2] < r0 else np.ascontiguousarray(X0)
    if Xt.shape != (n, d + 1, r0):
        raise ValueError("X0 gives tiles of shape %s, expected %s" % (Xt.shape, (n, d + 1, r0)))

    eval_every = 5  # sweeps between two evaluations of the stopping test
    r = r0
    ranges, graphs = build_pose_graphs(measurements, n, num_robots, r)
    plan = ExchangePlan(graphs)
    agents = [DeviceAgent(graphs, plan, a, Xt[s:e], ropt, device=device) for a, (s, e) in enumerate(ranges)]
    escapes: List[dict] = []
    sweeps: List[int] = []
    cert = None
    while True:
        if any(_in_robust_mode(ag) for ag in agents):
            raise ValueError("solveCertifiedDistributedPGO: robust (GNC) weights are not carried across a lift")
        cluster = RBCDCluster(plan, dict(enumerate(agents)))
        done = 0
        f, gn = cluster.team_cost_and_gradnorm()
        f_start, at_rest = f, False
        while gn > grad_tol and done < max_sweeps and not at_rest:
            for _ in range(min(eval_every, max_sweeps - done)):
                cluster.sweep()
                done += 1
            f_prev, gn_prev = f, gn
            f, gn = cluster.team_cost_and_gradnorm()
            at_rest = (f, gn) == (f_prev, gn_prev)  # (the same bits: the sweeps are deterministic, more change nothing)
        sweeps.append(done)
        if gn > grad_tol and not (at_rest and f < f_start):
            status = "NOT_CONVERGED_SWEEPS"
            break
        cert = certify_team(agents, **params)
        # NOT_CERTIFIED is decided by a Ritz value on the way; the escape needs the RETURNED pair to have negative curvature
        if cert.status == "NOT_CERTIFIED" and not cert.lambda_min < 0.0:
            status = "NOT_CONVERGED"
            break
        if cert.status in ("CERTIFIED", "NOT_CONVERGED"):
            status = cert.status
            break
        if r + 1 > r_max or not lib.dpgo_supported(d, r + 1):
            status = "RANK_LIMIT"
            break
        _ranges, graphs = build_pose_graphs(measurements, n, num_robots, r + 1)
        agents, plan, rec = escape_team(agents, cert.witness, graphs, grad_tol, ropt)
        rec.update(lambda_min=cert.lambda_min, gradnorm=cert.gradnorm, sweeps=done)  # (sweeps at the rank it leaves)
        escapes.append(rec)
        r += 1
    # round in the global frame (robot 0's first pose), evaluate the rounded trajectory on the same agents
    torch = agents[0].torch
    X = np.concatenate([ag.iterate_in_caller_order().cpu().numpy() for ag in agents])
    T = cluster.trajectories_in_global_frame()
    Tt = np.concatenate([T[a].cpu().numpy() for a in range(len(agents))])  # [n, d+1, d]
    keep = [ag.X.clone() for ag in agents]
    for ag, (s, e) in zip(agents, ranges):
        ag.set_iterate(lift_tiles(Tt[s:e], r))
    f_rounded, _gn = evaluate_team(agents)
    for ag, Xa in zip(agents, keep):
        ag.X.copy_(Xa)
    torch.cuda.synchronize(agents[0].device)
    return DistributedCertifiedPGOResult(np.asfortranarray(Tt.reshape(n * (d + 1), d).T), r, status, f, f_rounded,
                                         f_rounded - f, cert, np.asfortranarray(X.reshape(n * (d + 1), r).T), escapes,
                                         sweeps)
