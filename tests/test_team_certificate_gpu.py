"""The certificate of a TEAM's iterate from the agents' own blocks (dpgo_team_certify_device, k_cert_apply_team,
dpgo_amd.certificate.certify_team) against tests/certificate_reference.py on the assembled global problem.

The agents are DeviceAgents of the product (one handle each: Q_aa, the G coupling), side by side on one device; numpy
sees the oracle's global Q of the same measurements.  C(X) is defined at any X, so no test solves anything.  Bounds:
the apply tests' 1e-12 |ref|_F; check_pair's derived bounds for every returned pair; two runs of the same problem agree to
rho_1 + rho_2 + eps with rho = |C w - lam w|_2 from numpy (witness_figures), never the device's own residual.
gradnorm: 1e-12 relative to the central handle's, plus the suite's scalar floor 1e-12 |Q|_1 |X| (test_certificate_cases_gpu)
-- on a ring the gradient is zero and both figures are rounding.  DPGO_GRID_HESS forces second trips of the team kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest

import certificate_cases as K
import certificate_reference as ref
from certificate_cases import DR, ETA, TOL_REL, tile_poses
from conftest import DATA, ROOT, to_product_measurements

pytestmark = pytest.mark.gpu

_INST = {}


def _inst(key, make):
    if key not in _INST:
        _INST[key] = make()
    return _INST[key]


def uneven(n, k):
    """k uneven consecutive ranges of [0, n): sizes in the proportions 1 : 2 : ... : k (at least one pose each)."""
    cuts = np.round(np.cumsum(np.arange(1, k + 1)) / (k * (k + 1) / 2) * n).astype(int)
    cuts = np.maximum(cuts, np.arange(1, k + 1))
    cuts[-1] = n
    assert (np.diff(np.concatenate([[0], cuts])) > 0).all(), cuts
    return [(int(s), int(e)) for s, e in zip(np.concatenate([[0], cuts[:-1]]), cuts)]


def from_sizes(sizes):
    e = np.cumsum(sizes)
    return [(int(a), int(b)) for a, b in zip(np.concatenate([[0], e[:-1]]), e)]


class TeamOf:
    """DeviceAgents of the measurements `om` split by `ranges`, at the iterate X (r x (d+1)n); tweak(per_robot) may
    change the robots' measurement lists before the graphs are built."""

    def __init__(self, om, ranges, X, tweak=None, priors=None):
        import dpgo_amd
        from dpgo_amd.agent import DeviceAgent, ExchangePlan
        from dpgo_amd.measurements import partition_by_ranges
        d, r = om.d, X.shape[0]
        self.ranges, per_robot = partition_by_ranges(to_product_measurements(om), ranges)
        if tweak:
            tweak(per_robot)
        self.graphs = []
        for a, m in enumerate(per_robot):
            pg = dpgo_amd.PoseGraph(a, r, d)
            pg.setMeasurements(m)
            assert pg.n() == ranges[a][1] - ranges[a][0]
            self.graphs.append(pg)
        for a, idx in (priors or []):
            self.graphs[a].setPrior(idx, np.eye(r, d + 1))
        self.plan = ExchangePlan(self.graphs)
        Xt = K.tiles_of(X, d)
        self.agents = [DeviceAgent(self.graphs, self.plan, a, Xt[s:e]) for a, (s, e) in enumerate(self.ranges)]

    def certify(self, **kw):
        from dpgo_amd.certificate import certify_team
        res = certify_team(self.agents, **kw)
        print("  team of %d: %s lambda_min %.9e residual %.2e  %d its %d products  deflated %d  defect %.2e  %.1f ms" % (
            len(self.agents), res.status, res.lambda_min, res.residual, res.iterations, res.products, res.deflated,
            res.symmetry_defect, res.elapsedMs))
        return res


def probe_bound(d, N):
    return 8.0 * (d + 1) * N * 2.0 ** -53


def central(om, X, **kw):
    import dpgo_amd
    pg = dpgo_amd.PoseGraph(0, X.shape[0], om.d)
    pg.setMeasurements(to_product_measurements(om))
    return dpgo_amd.QuadraticProblem(pg).certify(X, **kw)


# ---------------------------------------------------------------- 1. the product
def _islands(oracle, d, sizes):
    """Three robots: robot 0 an island (no shared edge, no neighbour slot), robots 1 and 2 chains joined by edges from the
    first, a middle and the last pose of robot 1 to the FIRST and the LAST pose of robot 2."""
    rng = np.random.default_rng(77 + d)
    first = np.concatenate([[0], np.cumsum(sizes)])
    p1, p2 = [], []
    for a, n in enumerate(sizes):
        p1 += list(range(first[a], first[a] + n - 1))
        p2 += list(range(first[a] + 1, first[a] + n))
    lo1, hi1, lo2, hi2 = first[1], first[2] - 1, first[2], first[3] - 1
    p1 += [lo1, (lo1 + hi1) // 2, hi1, lo1]
    p2 += [lo2, hi2, hi2, hi2]
    m = len(p1)
    R = np.stack([np.linalg.qr(rng.standard_normal((d, d)))[0] for _ in range(m)])
    R[np.linalg.det(R) < 0, :, 0] *= -1
    z = np.zeros(m, dtype=np.int64)
    om = oracle.Measurements(d, z, np.array(p1, dtype=np.int64), z.copy(), np.array(p2, dtype=np.int64), R,
                             rng.standard_normal((m, d)), rng.uniform(5, 50, m), rng.uniform(5, 50, m), np.ones(m),
                             np.zeros(m, dtype=bool))
    return om, int(first[-1])


def _apply_case(oracle, om, n, ranges, r, label):
    from dpgo_amd.certificate import team_certificate_apply
    from test_launch_geometry_gpu import library_options
    d = om.d
    Qs = ref.sparse_Q(oracle.construct_Q(n, d, om))
    X = K.random_iterate(oracle, n, d, r, 31 + n + r)
    W = np.random.default_rng(5 + r).uniform(-1, 1, (r, (d + 1) * n))
    want = ref.certificate_apply(Qs, X, W, d)
    Cm = ref.certificate_matrix(Qs, X, d)
    got = {}
    for grid in (None, "1", "3"):
        with library_options({} if grid is None else {"DPGO_GRID_HESS": grid}):
            team = TeamOf(om, ranges, X)
            CW, wcw = team_certificate_apply(team.agents, K.tiles_of(W, d), gram=True)
            got[grid] = (K.matrix_of(CW), wcw)
    dev = got[None][0]
    err = np.linalg.norm(dev - want) / np.linalg.norm(want)
    # (the r x r block is summed workgroup by workgroup: its grouping, not the product, follows the grid)
    gerr = max(np.abs(wcw - W @ (Cm @ W.T)).max() for _, wcw in got.values()) / (ref.operator_norm1(Cm) * np.linalg.norm(W) ** 2)
    print("%s: |dev - ref|_F / |ref|_F %.2e   |W CW^T - numpy| / (|C|_1 |W|^2) %.2e" % (label, err, gerr))
    assert np.isfinite(dev).all() and err <= 1e-12
    assert gerr <= 1e-12
    for grid in ("1", "3"):
        assert np.array_equal(got[grid][0], dev), "DPGO_GRID_HESS=%s changes the product" % grid


@pytest.mark.parametrize("d,r", DR)
def test_team_apply(oracle, d, r):
    """N = 3 P + 5 poses split [1, P - 1, P, P + 1, rest]: a one-pose robot, ragged last tiles, tile-table boundaries that
    are no multiple of the tile; an island robot beside a pair whose slots hit the first and the last pose of the
    neighbour.  Forced grids of 1 and 3 workgroups give the same bits."""
    P = tile_poses(d)
    n = 3 * P + 5
    om, _, _ = K.random_graph(oracle, d, n, False)
    _apply_case(oracle, om, n, from_sizes([1, P - 1, P, P + 1, n - 3 * P - 1]), r, "%d-%d split" % (d, r))
    sizes = [P // 2 + 1, P + 3, 7]
    omi, ni = _inst(("islands", d), lambda: _islands(oracle, d, sizes))
    _apply_case(oracle, omi, ni, from_sizes(sizes), r, "%d-%d islands" % (d, r))


# ---------------------------------------------------------------- 2. verdicts
def _gn_close(team, cen, inst):
    floor = K.SCALAR_TOL * ref.operator_norm1(inst.Q) * np.linalg.norm(inst.X)
    assert abs(team.gradnorm - cen.gradnorm) <= 1e-12 * cen.gradnorm + floor, (team.gradnorm, cen.gradnorm)


def _verdict(inst, parts, status, deflated, lam_ref, prm, label):
    its = prm["max_iterations"]
    team = TeamOf(inst.om, uneven(inst.n, parts), inst.X)
    res = team.certify(**prm)
    cen = central(inst.om, inst.X, **prm)
    assert res.status == status == cen.status, (res, cen)
    assert res.deflated == deflated == cen.deflated, (res, cen)
    assert res.scale == cen.scale
    _gn_close(res, cen, inst)
    assert res.residual <= prm["tol_rel"] * res.scale and res.iterations < its, res
    assert res.symmetry_defect <= probe_bound(inst.d, inst.n), res.symmetry_defect
    Z = inst.Z(deflated)
    ft = K.check_pair(inst, Z, res.lambda_min, res.witness, lam_ref, True, prm["tol_rel"], label + " team")
    fc = K.witness_figures(inst, Z, cen.lambda_min, cen.witness)
    assert abs(res.lambda_min - cen.lambda_min) <= ft["rho"] + fc["rho"] + inst.eps, (res.lambda_min, cen.lambda_min, ft, fc)
    return res, ft


def _arbitrary(oracle, c, parts):
    inst = _inst(c, lambda: K.arbitrary(oracle, c))
    prm = dict(eta=ETA, tol_rel=TOL_REL, precond="none", max_iterations=K.budget(K.A_ITS))
    return _verdict(inst, parts, "NOT_CERTIFIED", 1, inst.lambda_ref(1), prm, "%s in %d" % (c.name, parts))


def _ring(oracle, c, winding, parts, **over):
    inst = _inst((c, winding), lambda: K.ring(oracle, c, winding))
    prm = dict(K.RING_PARAMS, max_iterations=K.budget(K.RING_ITS[c.n]))
    prm.update(over)
    want = K.ring_lambda(c) if winding else -K.ring_lambda(c)
    assert abs(inst.lambda_ref(c.d + 1) - want) <= 1e-10 * inst.scale
    res, f = _verdict(inst, parts, "NOT_CERTIFIED" if winding else "CERTIFIED", c.d + 1, want, prm,
                      "%s winding %d in %d" % (c.name, winding, parts))
    return inst, res, f


@pytest.mark.parametrize("k,dr", list(enumerate(DR)), ids=["%d-%d" % dr for dr in DR])
def test_team_verdicts(oracle, k, dr):
    """Group A (arbitrary X: NOT_CERTIFIED, t deflated) and group B (twisted ring: winding 1 NOT_CERTIFIED, winding 0
    CERTIFIED, d + 1 deflated) at P + 1 poses for every (d, r), in 2, 3 or 5 agents: status, deflated, scale and gradnorm
    of the central handle's certificate of the same X, the pair against numpy, lambda against the central one."""
    d, r = dr
    parts = (2, 3, 5)
    _arbitrary(oracle, K.Arbitrary(d, r, tile_poses(d) + 1, False), parts[k % 3])
    c = K.Ring(d, r, tile_poses(d) + 1)
    _ring(oracle, c, 1, parts[(k + 1) % 3])
    _ring(oracle, c, 0, parts[(k + 2) % 3])


def test_team_verdicts_200(oracle):
    """n = 200: several tiles per agent and agents smaller than a tile in one team."""
    _arbitrary(oracle, K.Arbitrary(3, 4, 200, False), 5)
    _arbitrary(oracle, K.Arbitrary(2, 3, 200, True), 3)
    _ring(oracle, K.Ring(3, 3, 200), 1, 2)
    _ring(oracle, K.Ring(2, 4, 200), 0, 5)


# ---------------------------------------------------------------- 3. preconditioners
@pytest.mark.parametrize("c", [K.Ring(3, 5, 200), K.Ring(2, 3, 257)], ids=lambda c: c.name)
def test_team_preconditioners_agree(oracle, c):
    """none, block-Jacobi and the members' V-cycles (2-D, r = 3: tiles of 9 doubles, slices the cycle takes through the
    staging buffers) in 4 agents: the same pair within rho_1 + rho_2 + eps."""
    got = []
    for precond in ("none", "jacobi", "multilevel"):
        inst, res, f = _ring(oracle, c, 1, 4, precond=precond)
        got.append((res, f))
    for res, f in got[1:]:
        assert abs(res.lambda_min - got[0][0].lambda_min) <= f["rho"] + got[0][1]["rho"] + inst.eps


# ---------------------------------------------------------------- 4. partitions, repeatability
def test_team_partition_independence_and_repeatability(oracle):
    c = K.Arbitrary(3, 5, 200, False)
    (a, fa), (b, fb) = _arbitrary(oracle, c, 2), _arbitrary(oracle, c, 5)
    inst = _INST[c]
    assert abs(a.lambda_min - b.lambda_min) <= fa["rho"] + fb["rho"] + inst.eps
    team = TeamOf(inst.om, uneven(inst.n, 3), inst.X)
    prm = dict(eta=ETA, tol_rel=TOL_REL, precond="jacobi", max_iterations=400)
    x, y = team.certify(**prm), team.certify(**prm)
    assert x.lambda_min == y.lambda_min and x.iterations == y.iterations and x.symmetry_defect == y.symmetry_defect
    assert np.array_equal(x.witness, y.witness)


# ---------------------------------------------------------------- 5. refusals, handle state
def test_team_refusals(oracle):
    import dpgo_amd
    import dpgo_amd.lib as L
    c = K.Arbitrary(3, 4, 200, False)
    inst = _inst(c, lambda: K.arbitrary(oracle, c))
    ranges = uneven(inst.n, 3)
    prm = dict(eta=ETA, tol_rel=TOL_REL, precond="none", max_iterations=20)
    with pytest.raises(ValueError, match="priors"):
        TeamOf(inst.om, ranges, inst.X, priors=[(1, 0)]).certify(**prm)

    def heavier(per_robot):  # robot 0's copy of its first shared edge: weight 1 -> 1 + 1e-3 (robot 1 keeps 1)
        m = per_robot[0]
        e = int(np.nonzero(m.r1 != m.r2)[0][0])
        m.weight[e] *= 1.0 + 1e-3
    with pytest.raises(dpgo_amd.DpgoError) as err:
        TeamOf(inst.om, ranges, inst.X, tweak=heavier).certify(**prm)
    assert err.value.code == L.ERR_STATE and "different weights or activity" in str(err.value), err.value
    team = TeamOf(inst.om, ranges, inst.X)
    team.agents[0].setRobotActive(1, False)
    with pytest.raises(dpgo_amd.DpgoError) as err:
        team.certify(**prm)
    assert err.value.code == L.ERR_STATE, err.value
    team.agents[0].setRobotActive(1, True)
    ok = team.certify(**prm)
    assert ok.symmetry_defect <= probe_bound(inst.d, inst.n), ok.symmetry_defect
    # member tables that do not tile [0, N), neighbours inside the own slice
    from dpgo_amd.certificate import _team_members, team_layout
    import ctypes as C
    import torch
    firsts, N, nbr = team_layout(team.agents)
    X = torch.cat([ag.X for ag in team.agents])
    cr, cp = L.TeamCertifyResultC(), dpgo_amd.certificate.certify_params(**prm)

    def rc(firsts, nbr):
        return L.load().dpgo_team_certify_device(_team_members(team.agents, firsts, nbr), len(firsts), L.ptr(X),
                                                 C.byref(cp), C.byref(cr), None)
    assert rc(firsts, nbr) == L.OK
    assert rc([0, firsts[1] + 1, firsts[2]], nbr) == L.ERR_INVALID
    bad = [v.copy() for v in nbr]
    bad[1][0] = firsts[1]  # inside robot 1's own slice
    assert rc(firsts, bad) == L.ERR_INVALID
    bad[1][0] = N
    assert rc(firsts, bad) == L.ERR_INVALID


def test_team_certify_leaves_the_agents_as_an_exchange_would(oracle):
    """A sweep after certify() gives the iterate of a sweep without it: certify only refreshes G (from the same X an
    exchange would deliver) and builds preconditioner data the solve rebuilds for itself."""
    from dpgo_amd.agent import RBCDCluster
    c = K.Arbitrary(3, 4, 200, False)
    inst = _inst(c, lambda: K.arbitrary(oracle, c))
    out = []
    for certify_first in (False, True):
        team = TeamOf(inst.om, uneven(inst.n, 3), inst.X)
        cluster = RBCDCluster(team.plan, dict(enumerate(team.agents)))
        if certify_first:
            res = cluster.certify(eta=ETA, tol_rel=TOL_REL, max_iterations=30)
            assert res.symmetry_defect is not None
        cluster.sweep()
        out.append(np.concatenate([ag.X.cpu().numpy() for ag in team.agents]))
    assert np.array_equal(out[0], out[1])


# ---------------------------------------------------------------- 6. one bigger case
def test_team_big_lattice(oracle):
    """synthetic_grid(21, 21, 21), r = 4, 8 agents of about 1 158 poses: 19 tiles each, 152 team tiles."""
    c = K.F_CASES[1]
    inst = _inst(c, lambda: K.big(oracle, c))
    if (1, 2) not in inst._ref:
        inst._ref[(1, 2)] = K.big_lambdas(inst, 1)
    its = K.budget(c.its)
    team = TeamOf(inst.om, uneven(inst.n, 8), inst.X)
    res = team.certify(eta=ETA, tol_rel=TOL_REL, precond="none", max_iterations=its)
    assert res.status == "NOT_CERTIFIED" and res.deflated == 1 and res.iterations < its, res
    assert res.residual <= TOL_REL * res.scale
    assert res.symmetry_defect <= probe_bound(inst.d, inst.n)
    K.check_pair(inst, inst.Z(1), res.lambda_min, res.witness, inst.lambda_ref(1), True, label=c.name + " team of 8")
    assert res.lambda_min < -ETA * res.scale


# ---------------------------------------------------------------- 7. the example
def test_example_certify_team_matches_certify():
    def status(flag):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "multi_robot_example.py"), "5",
                            os.path.join(DATA, "smallGrid3D.g2o"), flag], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("Certificate of the")]
        assert len(line) == 1, p.stdout[-2000:]
        return line[0].split(":")[1].split("|")[0].strip()
    assert status("--certify-team") == status("--certify")
