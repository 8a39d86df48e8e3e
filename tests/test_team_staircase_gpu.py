"""The staircase step of a TEAM (dpgo_team_eval_device, dpgo_team_escape_device, k_team_eval, k_cert_lift_retract;
dpgo_amd.certificate.evaluate_team / escape_team / solveCertifiedDistributedPGO) against
tests/team_staircase_reference.py on the assembled central problem.

Bounds: f to 1e-12 relative and |rgrad| to 1e-11 |EG| (test_problem_evaluations_match_oracle's), the rgrad tiles to 1e-12 in
Frobenius norm; X+ to RTOL_ELEM of tests/test_certificate_cases_gpu.py.  The figures of the 16-pose ring (LAM_RING, the
accepted first trial, f_after) are pinned on the reference alone by tests/test_team_staircase_reference_cpu.py."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import certificate_cases as K
import certificate_reference as ref
import team_staircase_reference as tsr
from certificate_cases import DR, tile_poses
from conftest import DATA, ROOT, to_product_measurements
from test_certificate_cases_gpu import RTOL_ELEM, Device
from test_team_certificate_gpu import TeamOf, _islands, from_sizes, uneven

pytestmark = pytest.mark.gpu

LAM_RING = -2.0 * (1.0 - math.cos(2.0 * math.pi / 16))


# ---------------------------------------------------------------- 1. evaluation
def _terms(team):
    import torch
    out = [ag.local_terms() for ag in team.agents]
    torch.cuda.synchronize()
    return out, [ag.X.cpu().numpy().copy() for ag in team.agents], [ag.nbr.cpu().numpy().copy() for ag in team.agents]


def _eval_case(oracle, om, n, ranges, r, label):
    from dpgo_amd.certificate import evaluate_team
    from test_launch_geometry_gpu import library_options
    d = om.d
    Qs = ref.sparse_Q(oracle.construct_Q(n, d, om))
    X = K.random_iterate(oracle, n, d, r, 53 + n + r)
    f_ref, rg_ref, _ = tsr.team_eval(Qs, X, d)
    eg = np.linalg.norm(np.asarray((Qs.T @ X.T).T))
    got = {}
    for grid in (None, "1", "3"):
        with library_options({} if grid is None else {"DPGO_GRID_HESS": grid}):
            team = TeamOf(om, ranges, X)
            before = _terms(team)
            f, gn, rg = evaluate_team(team.agents, gradient=True)
            f2, gn2 = evaluate_team(team.agents)
            after = _terms(team)
            assert (f, gn) == (f2, gn2), "two calls on one grid differ: %r %r" % ((f, gn), (f2, gn2))
            assert before[0] == after[0], "the agents' local terms changed"
            for x, y in zip(before[1] + before[2], after[1] + after[2]):
                assert np.array_equal(x, y), "the agents' X or neighbour buffers changed"
            got[grid] = (f, gn, K.matrix_of(rg))
    f, gn, rg = got[None]
    ef, eg_, er = abs(f - f_ref) / abs(f_ref), abs(gn - np.linalg.norm(rg_ref)) / eg, np.linalg.norm(rg - rg_ref) / np.linalg.norm(rg_ref)
    print("%s: |f - ref| / |ref| %.2e   | |rgrad| - ref | / |EG| %.2e   |rgrad - ref|_F / |ref|_F %.2e" % (label, ef, eg_, er))
    assert np.isfinite(rg).all() and ef <= 1e-12 and eg_ <= 1e-11 and er <= 1e-12
    for grid in ("1", "3"):
        assert np.array_equal(got[grid][2], rg), "DPGO_GRID_HESS=%s changes the gradient tiles" % grid
        assert abs(got[grid][0] - f) <= 1e-12 * abs(f) and abs(got[grid][1] - gn) <= 1e-12 * gn, (grid, got[grid][:2], f, gn)


@pytest.mark.parametrize("d,r", DR)
def test_team_eval(oracle, d, r):
    """An island beside a pair coupled through first and last poses (P + 1, 2P + 1, P - 1), a random graph of 3P + 2 poses
    in four uneven members, a chain with a one-pose member (1, P, P + 1); forced grids of 1 and 3 workgroups."""
    P = tile_poses(d)
    sizes = [P + 1, 2 * P + 1, P - 1]
    omi, ni = _islands(oracle, d, sizes)
    _eval_case(oracle, omi, ni, from_sizes(sizes), r, "%d-%d islands" % (d, r))
    n = 3 * P + 2
    om, _, _ = K.random_graph(oracle, d, n, False)
    _eval_case(oracle, om, n, uneven(n, 4), r, "%d-%d random" % (d, r))
    n = 2 * P + 2
    omc = K.chain_graph(oracle, d, n)[0]
    _eval_case(oracle, omc, n, from_sizes([1, P, P + 1]), r, "%d-%d chain" % (d, r))


# ---------------------------------------------------------------- 2. the escape against the central entry
def _escape_rc(team_next, r, X, w, grad_tol, Xn, firsts=None, agents=None):
    import dpgo_amd.lib as L
    from dpgo_amd.certificate import _team_members, team_layout
    f0, _N, nbr = team_layout(team_next.agents)
    out = L.TeamEscapeResultC()
    rc = L.load().dpgo_team_escape_device(_team_members(agents or team_next.agents, firsts or f0, nbr),
                                          len(team_next.agents), r, L.ptr(X), L.ptr(w), grad_tol, L.ptr(Xn), C.byref(out))
    return rc, out


def _escape_case(oracle, d, r, n, ranges, its):
    import torch
    import dpgo_amd.lib as L
    c = K.Ring(d, r, n)
    inst = K.ring(oracle, c, 1)
    team = TeamOf(inst.om, ranges, inst.X)
    res = team.certify(**dict(K.RING_PARAMS, max_iterations=K.budget(its)))
    assert res.status == "NOT_CERTIFIED", res
    w = res.witness.reshape(-1)
    nxt = TeamOf(inst.om, ranges, np.zeros((r + 1, inst.X.shape[1])))
    dev = team.agents[0].device
    X = torch.cat([ag.X for ag in team.agents]).contiguous()
    wd = torch.from_numpy(np.ascontiguousarray(w)).to(dev)
    Xn = torch.empty((n, d + 1, r + 1), dtype=torch.float64, device=dev)
    Xc = torch.empty_like(Xn)
    torch.cuda.synchronize()
    rc, out = _escape_rc(nxt, r, X, wd, 1e-9, Xn)
    L.check(rc)
    alpha_c = C.c_double(-1.0)
    with Device(inst, r + 1) as cen:
        L.check(cen.lib.dpgo_certify_escape_device(cen.h.h, r, L.ptr(X), L.ptr(wd), 1e-9, L.ptr(Xc), C.byref(alpha_c)))
        torch.cuda.synchronize()
    got, a = Xn.cpu().numpy(), out.alpha
    ratio = 0.1 * math.sqrt(n) / a
    k = int(round(math.log2(ratio)))
    assert a > 0 and 0 <= k < 60 and ratio == 2.0 ** k and out.trials == k + 1, (a, ratio, out.trials)
    f0, _, _ = tsr.team_eval(inst.Q, inst.X, d)
    f1, _, _ = tsr.team_eval(inst.Q, K.matrix_of(got), d)
    fc, _, _ = tsr.team_eval(inst.Q, K.matrix_of(Xc.cpu().numpy()), d)
    print("%s in %d: alpha %.4g (central %.4g, k = %d)  f %.9f -> %.9f  |rgrad| after %.2e" % (
        c.name, len(ranges), a, alpha_c.value, k, out.f_before, out.f_after, out.gradnorm_after))
    small = f0 - fc < 1e-9 * abs(f0)  # (the central call's accepted decrease is at rounding: its alpha may differ)
    assert not (small and n == 16), (f0, fc)
    if not small:
        assert a == alpha_c.value, (a, alpha_c.value)
    lifted = np.concatenate([K.tiles_of(inst.X, d), a * w.reshape(n, d + 1, 1)], axis=2)
    want = oracle.qf_retract(lifted, np.zeros_like(lifted), d)
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= RTOL_ELEM * np.abs(want).max(), np.abs(got - want).max()
    Y = got[:, :d, :]
    assert np.abs(Y @ np.swapaxes(Y, 1, 2) - np.eye(d)).max() <= 1e-12
    assert out.f_after < out.f_before
    assert abs(out.f_before - f0) <= 1e-12 * abs(f0) and abs(out.f_after - f1) <= 1e-12 * abs(f1), (out.f_before, f0, out.f_after, f1)


@pytest.mark.parametrize("d,r", K.LIFTS)
def test_team_escape_matches_central(oracle, d, r):
    """The winding-1 ring of 16 poses in 2 and in 4 uneven members and of P + 1 poses in 3: the team entry and
    dpgo_certify_escape_device on a central handle take the same alpha from the same X and witness."""
    _escape_case(oracle, d, r, 16, uneven(16, 2), K.RING_ITS[63])
    _escape_case(oracle, d, r, 16, uneven(16, 4), K.RING_ITS[63])
    n = tile_poses(d) + 1
    _escape_case(oracle, d, r, n, uneven(n, 3), K.RING_ITS[n])


def test_team_escape_refusals(oracle):
    """Every refusal is a return code decided on the host; the handles work afterwards."""
    import torch
    import dpgo_amd.lib as L
    d, r, n = 3, 3, 16
    inst = K.ring(oracle, K.Ring(d, r, n), 1)
    ranges = uneven(n, 2)
    team = TeamOf(inst.om, ranges, inst.X)
    nxt = TeamOf(inst.om, ranges, np.zeros((r + 1, inst.X.shape[1])))
    dev = team.agents[0].device
    X = torch.cat([ag.X for ag in team.agents]).contiguous()
    w = torch.from_numpy(np.random.default_rng(3).standard_normal(n * (d + 1))).to(dev)
    Xn = torch.full((n, d + 1, r + 1), np.nan, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    assert _escape_rc(nxt, r, X, w, 1e-9, Xn, agents=team.agents)[0] == L.ERR_INVALID  # rank-r members
    prior = TeamOf(inst.om, ranges, np.zeros((r + 1, inst.X.shape[1])), priors=[(1, 0)])
    assert _escape_rc(prior, r, X, w, 1e-9, Xn)[0] == L.ERR_INVALID
    assert _escape_rc(nxt, r, X, w, 1e-9, Xn, firsts=[ranges[1][0], 0])[0] == L.ERR_INVALID  # swapped slices
    assert _escape_rc(nxt, r, X, w, 1e-9, None)[0] == L.ERR_INVALID
    assert _escape_rc(nxt, r, X, w, -1.0, Xn)[0] == L.ERR_INVALID
    assert _escape_rc(nxt, r, X, w, float("nan"), Xn)[0] == L.ERR_INVALID
    for dd, rr in ((3, 6), (2, 5)):  # (d, r + 1) not compiled: the largest compiled rank has no next one
        top = K.ring(oracle, K.Ring(dd, rr, n), 1)
        t6 = TeamOf(top.om, ranges, top.X)
        X6 = torch.cat([ag.X for ag in t6.agents]).contiguous()
        w6 = torch.zeros(n * (dd + 1), dtype=torch.float64, device=dev)
        Xn6 = torch.empty((n, dd + 1, rr + 1), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        assert _escape_rc(t6, rr, X6, w6, 1e-9, Xn6)[0] == L.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(Xn).all(), "a refused call wrote X_next"
    res = team.certify(**dict(K.RING_PARAMS, max_iterations=K.budget(K.RING_ITS[63])))
    wd = torch.from_numpy(np.ascontiguousarray(res.witness.reshape(-1))).to(dev)
    rc, out = _escape_rc(nxt, r, X, wd, 1e-9, Xn)
    assert rc == L.OK and out.alpha > 0 and out.f_after < out.f_before, (rc, out.alpha)


# ---------------------------------------------------------------- 3. the driver
def _ring_meas(oracle, d):
    return to_product_measurements(K.ring_graph(oracle, d, 16)[0])


@pytest.mark.parametrize("robots", [2, 4])
@pytest.mark.parametrize("d", [2, 3])
def test_distributed_staircase_twisted_ring(oracle, d, robots):
    """From the winding-1 saddle at r0 = d the team escapes once or twice and certifies the global optimum f = 0."""
    import dpgo_amd
    res = dpgo_amd.solveCertifiedDistributedPGO(_ring_meas(oracle, d), 16, robots, X0=ref.ring_iterate(16, d, d, 1))
    print("d = %d, %d robots: %s at rank %d, f %.3e, sweeps per rank %s" % (d, robots, res.status, res.rank, res.f, res.sweeps))
    for e in res.escapes:
        print("  escape from rank %d: lambda_min %.9f alpha %.3g f %.9f -> %.9f after %d sweeps" % (
            e["rank"], e["lambda_min"], e["alpha"], e["f_before"], e["f_after"], e["sweeps"]))
    assert res.status == "CERTIFIED", res.status
    assert d + 1 <= res.rank <= d + 2 and len(res.escapes) == res.rank - d
    assert abs(res.escapes[0]["lambda_min"] - LAM_RING) <= 1e-8
    assert all(e["f_after"] < e["f_before"] for e in res.escapes)
    assert res.f <= 1e-10
    assert len(res.sweeps) == len(res.escapes) + 1 and max(res.sweeps) <= 500, res.sweeps
    T = np.ascontiguousarray(res.trajectory.T).reshape(16, d + 1, d)
    assert np.abs(T[:, :d, :] - T[0, :d, :]).max() <= 1e-5
    assert np.abs(T[0, :d, :] - np.eye(d)).max() <= 1e-12


def test_distributed_staircase_default_parameters_stall(oracle):
    """With the reference's local-solve defaults (radius 100, 3 RTR iterations) the team never leaves the escaped point:
    the reason for the driver's own defaults.  NOT_CONVERGED_SWEEPS, f where the first escape left it."""
    import dpgo_amd
    d = 3
    res = dpgo_amd.solveCertifiedDistributedPGO(_ring_meas(oracle, d), 16, 2, X0=ref.ring_iterate(16, d, d, 1),
                                                ropt=dpgo_amd.ROptParameters(), max_sweeps=50)
    print("default parameters: %s at rank %d, f %.12f (after the escape %.12f), sweeps %s" % (
        res.status, res.rank, res.f, res.escapes[0]["f_after"], res.sweeps))
    assert res.status == "NOT_CONVERGED_SWEEPS" and res.rank == d + 1 and len(res.escapes) == 1
    assert res.sweeps[0] == 0 and 0 < res.sweeps[1] <= 50, res.sweeps  # (it stops as soon as the sweeps repeat themselves)
    assert res.f == res.escapes[0]["f_after"]


def test_distributed_staircase_smallgrid():
    import dpgo_amd
    meas, n = dpgo_amd.read_g2o_file(os.path.join(DATA, "smallGrid3D.g2o"))
    res = dpgo_amd.solveCertifiedDistributedPGO(meas, n, 5)
    print("smallGrid3D in 5: %s at rank %d, 2 f_rounded %.10f, sweeps %s" % (res.status, res.rank, 2 * res.f_rounded, res.sweeps))
    assert res.status == "CERTIFIED" and res.rank == 3 and res.escapes == []
    assert abs(2 * res.f_rounded - 1025.3980556263) <= 1e-6 * 1025.3980556263


def test_example_staircase(tmp_path):
    g2o = tmp_path / "ring.g2o"
    g2o.write_text("".join("EDGE_SE2 %d %d 0 0 0 1 0 0 1 0 1\n" % (i, (i + 1) % 16) for i in range(16)))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "multi_robot_example.py"), "2", str(g2o),
                        "--staircase"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "CERTIFIED" in p.stdout.strip().splitlines()[-1].replace("NOT_CERTIFIED", ""), p.stdout[-2000:]
