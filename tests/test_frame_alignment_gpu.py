"""Robust frame alignment on the device (kernels/align.h) against the NumPy restatement in fp64 and longdouble
(tests/frame_alignment_reference.py): the averaging kernel, candidates and lift, and the protocol end to end.

Tolerance rule (frame_alignment_reference.allowed_error): a device result may be off the LONGDOUBLE run by 32 times the
error of the fp64 NumPy restatement on the same input -- the device contracts to fma and sums in another order, a few
ulps per operation over about 35 GNC iterations --, and not below 1e-14 max(1, |t|).  Every test prints the device's
and NumPy's error before it asserts.

Measured on an MI355X (largest over the groups / cases of a test: device error / NumPy error, both against longdouble):
  averaging kernel    d=2 two-stage 1.1e-15 / 5.6e-15    d=2 pose 8.9e-16 / 3.2e-15
                      d=3 two-stage 8.0e-16 / 4.8e-15    d=3 pose 1.9e-15 / 3.6e-15      (allowed: 5.7e-14 .. 1.5e-13)
  candidates          2.1e-14 .. 3.9e-14 / 2.2e-14 .. 3.9e-14 over the eight (d, r), entries up to 150 (allowed 1.3e-12 .. 1.6e-12)
  lift                8.7e-15 .. 2.0e-14 / 8.7e-15 .. 1.5e-14                                    (allowed 6.7e-13 .. 9.4e-13)
  protocol, case (a)  X of robots 1 .. 3: 1.0e-15 .. 1.4e-15 / 1.4e-15 .. 2.7e-15 (allowed 4.4e-14 .. 8.6e-14), 2.4e-15 .. 3.5e-15
                      from the ground truth; central cost 0.0 aligned against 4.2e+02 lifted without alignment
  protocol, case (b)  transform of robot 2: 1.1e-15 / 9.5e-16 (allowed 3.0e-14), 8.7e-04 from the clean data's
"""
import ctypes as C
import gc

import numpy as np
import pytest

import frame_alignment_reference as F
from manifold_reference import DR, LD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import dpgo_amd
    import dpgo_amd.lib as L
    return torch, L, L.load(), dpgo_amd


def _dev(torch, a, dtype=None):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _records(L, t):
    raw = t.cpu().numpy().tobytes()
    return list((L.AverageResultC * (len(raw) // C.sizeof(L.AverageResultC))).from_buffer_copy(raw))


def _params(L, lib, mode, **kw):
    p = L.AverageParamsC()
    lib.dpgo_average_params_default(mode, C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _tile(rec, d):
    return np.array(rec.T[:(d + 1) * d]).reshape(d + 1, d)


def _average_device(env, d, mode, tiles, gp):
    torch, L, lib, _ = env
    ng = len(gp) - 1
    cand, gpd = _dev(torch, tiles, torch.float64), _dev(torch, gp, torch.int32)
    w = torch.full((max(len(tiles), 1),), -7.0, dtype=torch.float64, device="cuda")
    res = torch.zeros((ng, C.sizeof(L.AverageResultC)), dtype=torch.uint8, device="cuda")
    prm = _params(L, lib, mode)
    L.check(lib.dpgo_robust_average_device(d, ng, L.ptr(gpd), L.ptr(cand), None, None, C.byref(prm), L.ptr(w), L.ptr(res), None))
    torch.cuda.synchronize()
    return res.cpu().numpy().copy(), w.cpu().numpy().copy(), _records(L, res)


# ---------------------------------------------------------------- 1. the averaging kernel
EMPTY_AT = 3  # an empty group in the middle of the launch


@pytest.mark.parametrize("mode", [F.TWO_STAGE, F.POSE])
@pytest.mark.parametrize("d", [2, 3])
def test_robust_average_kernel(env, d, mode):
    """One launch over the eight groups (1/1 .. 300/600 inliers of candidates, 64 / 65 / 257 among them) and an empty one:
    status, inlier set, iteration count and the decided weights are the fp64 restatement's, the transform is the
    longdouble run's within the tolerance rule; a second launch and the host flavour give the same bits; one NaN makes its
    group INVALID and changes nothing else."""
    torch, L, lib, _ = env
    case, r64, rld = F.reference_runs(d, mode)
    tiles = np.ascontiguousarray(F.to_tiles(case["R"], case["t"]))
    gp = np.insert(case["group_ptr"], EMPTY_AT, case["group_ptr"][EMPTY_AT]).astype(np.int32)
    assert gp[-1] == 1042 and len(gp) == 10
    raw, w, recs = _average_device(env, d, mode, tiles, gp)
    groups = [g for g in range(9) if g != EMPTY_AT]
    assert recs[EMPTY_AT].status == F.EMPTY and recs[EMPTY_AT].candidates == 0
    worst_dev = worst_np = 0.0
    for k, g in enumerate(groups):
        a, b, rec = r64[k], rld[k], recs[g]
        lo, hi = gp[g], gp[g + 1]
        t64, tld = F.to_tiles(a["R"][None], a["t"][None])[0], F.to_tiles(b["R"][None], b["t"][None])[0]
        err_np = float(np.max(np.abs(t64 - tld)))
        err_dev = float(np.max(np.abs(_tile(rec, d).astype(LD) - tld)))
        allowed = F.allowed_error(err_np, float(np.sqrt(np.sum(b["t"] ** 2))))
        print("d=%d mode=%d group %d (%d candidates): status %d, %d inliers, %d iterations, mu %.3e | device error %.3e, "
              "NumPy error %.3e, allowed %.3e" % (d, mode, g, hi - lo, rec.status, rec.inliers, rec.iterations, rec.mu,
                                                  err_dev, err_np, allowed))
        worst_dev, worst_np = max(worst_dev, err_dev), max(worst_np, err_np)
        assert rec.status == a["status"] and rec.candidates == hi - lo
        assert list(np.nonzero(w[lo:hi] > 1 - F.W_TOL)[0]) == list(a["inliers"]) and rec.inliers == len(a["inliers"])
        assert rec.iterations == a["iterations"]
        for v in (0.0, 1.0):
            assert (w[lo:hi][a["weights"] == v] == v).all()
        assert abs(rec.mu - float(a["mu"])) <= 1e-12 * abs(float(a["mu"]))
        assert err_dev <= allowed
    print("d=%d mode=%d: largest device error %.3e, largest NumPy error %.3e" % (d, mode, worst_dev, worst_np))
    # the same bits from a second launch and from the host flavour
    raw2, w2, _ = _average_device(env, d, mode, tiles, gp)
    assert raw2.tobytes() == raw.tobytes() and w2.tobytes() == w.tobytes()
    wh = np.zeros(len(tiles))
    resh = (L.AverageResultC * 9)()
    prm = _params(L, lib, mode)
    L.check(lib.dpgo_robust_average(d, 9, L.ptr(gp), L.ptr(tiles), None, None, C.byref(prm), L.ptr(wh),
                                    C.addressof(resh), 0))
    assert bytes(resh) == raw.tobytes() and wh.tobytes() == w.tobytes()
    # one NaN entry: its group is INVALID, its neighbours in the launch are untouched
    bad_g = 6  # the 33 / 65 group
    bad = tiles.copy()
    bad[gp[bad_g] + 40, d, 0] = np.nan
    raw3, w3, recs3 = _average_device(env, d, mode, bad, gp)
    assert recs3[bad_g].status == F.INVALID and recs3[bad_g].iterations == 0
    assert (w3[gp[bad_g]:gp[bad_g + 1]] == 0).all()
    for g in range(9):
        if g != bad_g:
            assert raw3[g].tobytes() == raw[g].tobytes() and w3[gp[g]:gp[g + 1]].tobytes() == w[gp[g]:gp[g + 1]].tobytes()


def test_robust_average_arguments(env):
    """DPGO_ERR_INVALID before any launch: null / misaligned pointers, d outside {2, 3}, non-positive barc / mu_step / w_tol,
    a decreasing group_ptr in the host flavour; the Python counterparts of the reference's two functions."""
    torch, L, lib, _ = env
    from dpgo_amd.initialization import angular2ChordalSO3, robustSinglePoseAveraging, robustSingleRotationAveraging
    case, r64, _ = F.reference_runs(3, F.TWO_STAGE)
    gp = case["group_ptr"]
    tiles = np.ascontiguousarray(F.to_tiles(case["R"], case["t"]))
    w, res = np.zeros(len(tiles)), (L.AverageResultC * 8)()
    prm = _params(L, lib, F.TWO_STAGE)
    args = lambda **kw: [kw.get("d", 3), 8, L.ptr(kw.get("gp", gp)), L.ptr(tiles), None, None,
                         C.byref(kw.get("prm", prm)), L.ptr(w), C.addressof(res), 0]
    assert lib.dpgo_robust_average(*args()) == L.OK
    assert lib.dpgo_robust_average(*args(d=4)) == L.ERR_INVALID
    dec = gp.copy()
    dec[3] = dec[2] - 1
    assert lib.dpgo_robust_average(*args(gp=dec)) == L.ERR_INVALID
    for field in ("barc", "mu_step", "w_tol"):
        assert lib.dpgo_robust_average(*args(prm=_params(L, lib, F.TWO_STAGE, **{field: 0.0}))) == L.ERR_INVALID
    cand = _dev(torch, np.concatenate([tiles.reshape(-1), [0.0]]), torch.float64)
    gpd, wd = _dev(torch, gp, torch.int32), torch.zeros(len(tiles) + 1, dtype=torch.float64, device="cuda")
    resd = torch.zeros((8, C.sizeof(L.AverageResultC)), dtype=torch.uint8, device="cuda")
    dev = lambda c, ww, rr: lib.dpgo_robust_average_device(3, 8, L.ptr(gpd), c, None, None, C.byref(prm), ww, rr, None)
    assert dev(None, L.ptr(wd), L.ptr(resd)) == L.ERR_INVALID
    assert dev(L.ptr(cand) + 4, L.ptr(wd), L.ptr(resd)) == L.ERR_INVALID
    assert dev(L.ptr(cand), L.ptr(wd) + 2, L.ptr(resd)) == L.ERR_INVALID
    assert dev(L.ptr(cand), L.ptr(wd), L.ptr(resd)) == L.OK
    torch.cuda.synchronize()
    ref = _records(L, resd)
    # pointers offset by 8 bytes are accepted and give the same bits (the header's alignment paragraph)
    cand8 = torch.zeros(tiles.size + 1, dtype=torch.float64, device="cuda")
    cand8[1:] = cand[:-1]
    res8, w8 = torch.zeros_like(resd), torch.zeros_like(wd)
    assert dev(L.ptr(cand8[1:]), L.ptr(w8[1:]), L.ptr(res8)) == L.OK
    torch.cuda.synchronize()
    assert res8.cpu().numpy().tobytes() == resd.cpu().numpy().tobytes() and torch.equal(w8[1:], wd[:-1])
    assert [r.inliers for r in ref] == [len(a["inliers"]) for a in r64]
    # the reference's signatures
    g = 5
    Rg, tg = case["R"][gp[g]:gp[g + 1]], case["t"][gp[g]:gp[g + 1]]
    ROpt, inl = robustSingleRotationAveraging(list(Rg), np.ones(len(Rg)), angular2ChordalSO3(0.5))
    assert inl == list(r64[g]["inliers"]) and np.max(np.abs(ROpt - r64[g]["R"])) <= 1e-13
    pose = F.robust_single_pose_averaging(Rg, tg, 10000.0, 100.0, np.sqrt(F.CHI2INV_09_3))
    ROpt, tOpt, inl = robustSinglePoseAveraging(list(Rg), list(tg), np.zeros(0), np.zeros(0), np.sqrt(F.CHI2INV_09_3))
    assert inl == list(pose["inliers"]) and np.max(np.abs(ROpt - pose["R"])) <= 1e-13 and np.max(np.abs(tOpt - pose["t"])) <= 1e-12


# ---------------------------------------------------------------- 2. candidates and lift
def _record_bytes(L, status, T, d):
    rec = L.AverageResultC()
    rec.status, rec.inliers, rec.candidates = status, 5, 9
    for q, v in enumerate(np.asarray(T, dtype=np.float64).reshape(-1)):
        rec.T[q] = v
    return np.frombuffer(bytes(rec), dtype=np.uint8).copy()


@pytest.mark.parametrize("d,r", DR)
def test_candidates_and_lift(env, d, r):
    """Every (d, r) the library compiles, both edge directions: 300 edges over 40 local poses and 70 neighbour slots, a
    random YLift in St(d, r), translations up to 50; candidates and the lifted X against longdouble; a failed record leaves
    X bitwise untouched; buffers offset by 8 bytes give the same bits."""
    torch, L, lib, _ = env
    assert lib.dpgo_supported(d, r)
    rng = np.random.Generator(np.random.PCG64([7, d, r]))
    m, n, slots = 300, 40, 70
    Y = np.linalg.qr(rng.standard_normal((r, d)))[0]
    ident = F.to_tiles(np.eye(d)[None], np.zeros((1, d)))[0]
    Xn = np.asarray(F.lift_in_frame(Y, ident, F.to_tiles(F.random_rotations(rng, slots, d), rng.uniform(-50, 50, (slots, d)))),
                    dtype=np.float64)
    Tl = F.to_tiles(F.random_rotations(rng, n, d), rng.uniform(-50, 50, (n, d)))
    my, sl = rng.integers(0, n, m).astype(np.int32), rng.integers(0, slots, m).astype(np.int32)
    inc = (np.arange(m) % 2).astype(np.uint8)
    Re, te = F.random_rotations(rng, m, d), rng.uniform(-50, 50, (m, d))
    Yc = np.ascontiguousarray(Y.T)  # r x d column-major
    f64 = lambda a, pad=0: _dev(torch, np.concatenate([np.zeros(pad), np.asarray(a, dtype=np.float64).reshape(-1)]), torch.float64)
    outs = []
    myd, sld, incd = _dev(torch, my, torch.int32), _dev(torch, sl, torch.int32), _dev(torch, inc, torch.uint8)
    for pad in (0, 1):  # pad = 1: every double buffer starts 8 bytes into its allocation
        Tld, Xnd, Rd, td = f64(Tl, pad), f64(Xn, pad), f64(Re, pad), f64(te, pad)
        cand = torch.zeros(m * (d + 1) * d + pad, dtype=torch.float64, device="cuda")
        L.check(lib.dpgo_neighbor_candidates_device(r, d, m, L.ptr(Yc), L.ptr(Tld[pad:]), L.ptr(Xnd[pad:]), L.ptr(myd),
                                                    L.ptr(sld), L.ptr(incd), L.ptr(Rd[pad:]), L.ptr(td[pad:]),
                                                    L.ptr(cand[pad:]), None))
        torch.cuda.synchronize()
        outs.append(cand[pad:].cpu().numpy().reshape(m, d + 1, d))
    assert outs[0].tobytes() == outs[1].tobytes()
    c64 = F.neighbor_transforms(Y, Xn, Tl, my, sl, inc, Re, te, np.float64)
    cld = F.neighbor_transforms(Y, Xn, Tl, my, sl, inc, Re, te, LD)
    err_np, err_dev = float(np.max(np.abs(c64 - cld))), float(np.max(np.abs(outs[0].astype(LD) - cld)))
    allowed = F.allowed_error(err_np, float(np.max(np.abs(cld[:, d, :]))))
    print("(d, r) = (%d, %d) candidates: device error %.3e, NumPy error %.3e, allowed %.3e" % (d, r, err_dev, err_np, allowed))
    assert err_dev <= allowed
    # the lift: from a record in device memory, from the host's transform, and not at all for a failed record
    Tw = np.ascontiguousarray(F.to_tiles(F.random_rotations(rng, 1, d), rng.uniform(-50, 50, (1, d)))[0])
    X0 = rng.standard_normal((n, d + 1, r))
    res = []
    for pad in (0, 1):
        Tld = f64(Tl, pad)
        for status, host in ((F.OK, False), (F.OK, True), (F.FEW_INLIERS, False), (F.INVALID, False), (F.EMPTY, False)):
            X = f64(X0, pad)
            rec = _dev(torch, _record_bytes(L, status, Tw, d), torch.uint8)
            L.check(lib.dpgo_lift_in_frame_device(r, d, n, L.ptr(Yc), L.ptr(Tld[pad:]), None if host else L.ptr(rec),
                                                  L.ptr(Tw) if host else None, L.ptr(X[pad:]), None))
            torch.cuda.synchronize()
            got = X[pad:].cpu().numpy().reshape(n, d + 1, r)
            if status == F.OK:
                res.append(got)
            else:
                assert got.tobytes() == X0.tobytes()
    assert all(x.tobytes() == res[0].tobytes() for x in res)
    x64, xld = F.lift_in_frame(Y, Tw, Tl, np.float64), F.lift_in_frame(Y, Tw, Tl, LD)
    err_np, err_dev = float(np.max(np.abs(x64 - xld))), float(np.max(np.abs(res[0].astype(LD) - xld)))
    allowed = F.allowed_error(err_np, float(np.max(np.abs(xld[:, d, :]))))
    print("(d, r) = (%d, %d) lift: device error %.3e, NumPy error %.3e, allowed %.3e" % (d, r, err_dev, err_np, allowed))
    assert err_dev <= allowed
    # both sources or none: rejected before any launch
    X, Tld = f64(X0), f64(Tl)
    assert lib.dpgo_lift_in_frame_device(r, d, n, L.ptr(Yc), L.ptr(Tld), None, None, L.ptr(X), None) == L.ERR_INVALID
    assert lib.dpgo_lift_in_frame_device(r + 7, d, n, L.ptr(Yc), L.ptr(Tld), None, L.ptr(Tw), L.ptr(X), None) == L.ERR_UNSUPPORTED


# ---------------------------------------------------------------- 3. the protocol end to end
R_LIFT = 5


def _noise_free(dpgo_amd, p1, p2, Ttrue):
    """Measurements p1 -> p2 from the ground-truth tiles [n, d+1, d] with kappa = tau = 1."""
    d = Ttrue.shape[2]
    Rt, tt = F.from_tiles(Ttrue)
    Rij, tij = F.se_compose(*F.se_inverse(Rt[p1], tt[p1]), Rt[p2], tt[p2])
    m = len(p1)
    return dpgo_amd.RelativeSEMeasurements(d, np.zeros(m), p1, np.zeros(m), p2, Rij, tij, np.ones(m), np.ones(m), np.ones(m),
                                           p1 + 1 == p2)


def _lattice(dpgo_amd, corrupt=None):
    """4 x 4 x 4 noise-free lattice in snake order, four robots of 16 poses (one z layer each: a chain 0-1-2-3 with 16
    shared loop closures per link).  corrupt = (a, b, count, seed): `count` of the closures between robots a and b are
    replaced by random rigid transforms.  Returns (measurements, Ttrue, corrupted (p1, p2) pairs)."""
    from dpgo_amd.synthetic import synthetic_grid
    meas, n, Ttrue = synthetic_grid(4, 4, 4, seed=3)
    meas = _noise_free(dpgo_amd, meas.p1.copy(), meas.p2.copy(), Ttrue)
    bad = []
    if corrupt is not None:
        a, b, count, seed = corrupt
        rng = np.random.Generator(np.random.PCG64(seed))
        link = np.nonzero((meas.p1 // 16 == a) & (meas.p2 // 16 == b))[0]
        assert len(link) == 16
        for e in rng.choice(link, count, replace=False):
            meas.R[e] = F.random_rotations(rng, 1, 3)[0]
            meas.t[e] = rng.uniform(-5, 5, 3)
            bad.append((int(meas.p1[e]), int(meas.p2[e])))
    return meas, n, Ttrue, bad


def _local_frames(dpgo_amd, graphs):
    from dpgo_amd.initialization import odometry_initialization
    out = []
    for a, pg in enumerate(graphs):
        m = pg.measurements()
        odo = m.select((m.r1 == a) & (m.r2 == a) & (m.p1 + 1 == m.p2))
        out.append(odometry_initialization(odo, pg.n()))
    return out


def _team(dpgo_amd, meas, n, robots):
    from dpgo_amd.agent import DeviceAgent, ExchangePlan, RBCDCluster, build_pose_graphs
    ranges, graphs = build_pose_graphs(meas, n, robots, R_LIFT)
    plan = ExchangePlan(graphs)
    local = _local_frames(dpgo_amd, graphs)
    agents = {a: DeviceAgent.from_local_frame(graphs, plan, a, local[a]) for a in range(robots)}
    return ranges, graphs, plan, local, agents, RBCDCluster(plan, agents)


def _protocol_reference(graphs, plan, local, dt, unit_weights=False):
    """The whole protocol on the host: {agent: X tiles}, {agent: (neighbour, run)} -- rounds, ascending neighbour order, the
    first success initialises (RBCDCluster.initialize_in_global_frame)."""
    d = graphs[0].d()
    Y = np.eye(R_LIFT, d)
    ident = F.to_tiles(np.eye(d)[None], np.zeros((1, d)))[0]
    X = {0: F.lift_in_frame(Y, ident, local[0], dt)}
    runs = {}
    while len(X) < len(graphs):
        ready, progress = set(X), False
        for a in range(len(graphs)):
            if a in X:
                continue
            m = graphs[a].sharedLoopClosures()
            for q in plan.adj[a]:
                if q not in ready:
                    continue
                out = m.r1 == a
                sel = np.nonzero(np.where(out, m.r2, m.r1) == q)[0]
                nbr = np.stack([X[q][int(m.p2[e] if out[e] else m.p1[e])] for e in sel])
                cand = F.neighbor_transforms(Y, nbr, local[a], np.where(out, m.p1, m.p2)[sel], np.arange(len(sel)), ~out[sel],
                                             m.R[sel], m.t[sel], dt)
                run = F.robust_transform(*F.from_tiles(cand), F.TWO_STAGE, dt, unit_weights=unit_weights)
                runs[a] = (q, run, sel)
                if run["status"] == F.OK:
                    X[a] = F.lift_in_frame(Y, F.to_tiles(run["R"][None], run["t"][None])[0], local[a], dt)
                    progress = True
                    break
        if not progress:
            break
    return X, runs


def _truth_in_frame_of_robot0(Ttrue):
    Rt, tt = F.from_tiles(Ttrue.astype(LD))
    Rg, tg = F.se_compose(*F.se_inverse(Rt[:1], tt[:1]), Rt, tt)
    return F.lift_in_frame(np.eye(R_LIFT, 3), F.to_tiles(np.eye(3)[None], np.zeros((1, 3)))[0], F.to_tiles(Rg, tg), LD)


def test_protocol_aligns_a_noise_free_lattice(env):
    """Case (a): four robots that know only their own odometry end in the frame of robot 0: X is the lifted ground truth,
    the central cost of the aligned start is a rounding residue of the unaligned one's, and the sweeps run."""
    torch, L, lib, dpgo_amd = env
    meas, n, Ttrue, _ = _lattice(dpgo_amd)
    ranges, graphs, plan, local, agents, cluster = _team(dpgo_amd, meas, n, 4)
    assert cluster.waiting_agents() == [1, 2, 3]
    records, waiting = cluster.initialize_in_global_frame()
    assert waiting == [] and all(ag.state == "INITIALIZED" for ag in agents.values())
    assert {a: (r.neighbour, r.status, r.inliers, r.candidates) for a, r in records.items()} == {
        1: (0, "OK", 16, 16), 2: (1, "OK", 16, 16), 3: (2, "OK", 16, 16)}
    x64, _ = _protocol_reference(graphs, plan, local, np.float64)
    xld, _ = _protocol_reference(graphs, plan, local, LD)
    truth = _truth_in_frame_of_robot0(Ttrue)
    for a in range(4):
        got = agents[a].X.cpu().numpy().astype(LD)
        err_np, err_dev = float(np.max(np.abs(x64[a] - xld[a]))), float(np.max(np.abs(got - xld[a])))
        allowed = F.allowed_error(err_np, float(np.max(np.abs(xld[a][:, 3, :]))))
        print("robot %d: device error %.3e, NumPy error %.3e, allowed %.3e, distance to the truth %.3e" % (
            a, err_dev, err_np, allowed, float(np.max(np.abs(got - truth[ranges[a][0]:ranges[a][1]])))))
        assert err_dev <= allowed
        assert float(np.max(np.abs(got - truth[ranges[a][0]:ranges[a][1]]))) <= 1e-12
    aligned = cluster.central_cost_and_gradnorm()[0]
    _, _, _, _, agents0, cluster0 = _team(dpgo_amd, meas, n, 4)
    for ag in agents0.values():
        if ag.state != "INITIALIZED":
            ag.initializeInGlobalFrame()  # every robot keeps its own frame
    unaligned = cluster0.central_cost_and_gradnorm()[0]
    print("central cost: aligned %.3e, lifted without alignment %.3e" % (aligned, unaligned))
    assert unaligned > 1.0 and abs(aligned) < 1e-12 * unaligned
    for _ in range(3):
        cluster.sweep()
    assert np.isfinite(cluster.central_cost_and_gradnorm()[0])


def test_protocol_rejects_outlier_loop_closures(env):
    """Case (b): 5 of the 16 closures between robots 1 and 2 are random rigid transforms: robot 2 finds 11 inliers of 16, the
    planted weights and the restatement's transform within the tolerance rule.  Against the transform of the clean data it
    is off by 9e-4, in the restatement too: the estimate returned is the one of GNC's LAST solve, whose weights were not yet
    all decided (src/DPGO_solver.cpp:107-125) -- below the 1e-2 by which the restatement with every weight forced to 1
    misses it (0.48 here), so the test can tell a robust average from a plain one."""
    torch, L, lib, dpgo_amd = env
    meas, n, Ttrue, bad = _lattice(dpgo_amd, corrupt=(1, 2, 5, 11))
    ranges, graphs, plan, local, agents, cluster = _team(dpgo_amd, meas, n, 4)
    records, waiting = cluster.initialize_in_global_frame()
    assert waiting == []
    rec = records[2]
    assert (rec.neighbour, rec.status, rec.inliers, rec.candidates) == (1, "OK", 11, 16)
    x64, r64 = _protocol_reference(graphs, plan, local, np.float64)
    xld, rld = _protocol_reference(graphs, plan, local, LD)
    q, run, sel = rld[2]
    m = graphs[2].sharedLoopClosures()
    planted = np.array([0.0 if (int(m.p1[e]) + 16, int(m.p2[e]) + 32) in bad else 1.0 for e in sel])
    assert q == 1 and planted.sum() == 11
    w = agents[2].alignment_weights(1)
    assert (w == planted).all() and (np.asarray(run["weights"], dtype=np.float64) == planted).all()
    tld = F.to_tiles(run["R"][None], run["t"][None])[0]
    t64 = F.to_tiles(r64[2][1]["R"][None], r64[2][1]["t"][None])[0]
    err_np, err_dev = float(np.max(np.abs(t64 - tld))), float(np.max(np.abs(rec.T_world_robot.astype(LD) - tld)))
    allowed = F.allowed_error(err_np, float(np.sqrt(np.sum(run["t"] ** 2))))
    Rt, tt = F.from_tiles(Ttrue.astype(LD))
    want = F.to_tiles(*F.se_compose(*F.se_inverse(Rt[:1], tt[:1]), Rt[32:33], tt[32:33]))[0]  # robot 2's pose 0 in robot 0's frame
    print("robot 2 from robot 1: device error %.3e, NumPy error %.3e, allowed %.3e, distance to the clean transform %.3e" % (
        err_dev, err_np, allowed, float(np.max(np.abs(rec.T_world_robot - want)))))
    assert err_dev <= allowed
    assert float(np.max(np.abs(rec.T_world_robot - want))) < 1e-2
    _, plain = _protocol_reference(graphs, plan, local, np.float64, unit_weights=True)
    off = F.to_tiles(plain[2][1]["R"][None], plain[2][1]["t"][None])[0] - np.asarray(want, dtype=np.float64)
    assert float(np.max(np.abs(off))) > 1e-2


def test_protocol_leaves_an_agent_waiting(env):
    """Case (c): two robots with a single shared edge and min_inliers = 2: robot 1 stays in WAIT_FOR_INITIALIZATION, is
    returned in the waiting list, keeps its X bit for bit, and a sweep refuses to run."""
    torch, L, lib, dpgo_amd = env
    rng = np.random.Generator(np.random.PCG64(5))
    Ttrue = F.to_tiles(F.random_rotations(rng, 8, 3), rng.uniform(-3, 3, (8, 3)))
    p1 = np.arange(7)
    meas = _noise_free(dpgo_amd, p1, p1 + 1, Ttrue)  # a chain: the edge 3 -> 4 is the only one the robots share
    ranges, graphs, plan, local, agents, cluster = _team(dpgo_amd, meas, 8, 2)
    agents[1].X.copy_(torch.tensor(rng.standard_normal((4, 4, R_LIFT)), device="cuda"))
    before = agents[1].X.cpu().numpy().copy()
    records, waiting = cluster.initialize_in_global_frame(min_inliers=2)
    assert waiting == [1] and agents[1].state == "WAIT_FOR_INITIALIZATION"
    assert (records[1].status, records[1].inliers, records[1].candidates) == ("FEW_INLIERS", 1, 1)
    assert agents[1].X.cpu().numpy().tobytes() == before.tobytes()
    with pytest.raises(RuntimeError, match="WAIT_FOR_INITIALIZATION"):
        cluster.sweep()
    with pytest.raises(RuntimeError, match="WAIT_FOR_INITIALIZATION"):
        cluster.phase(0)
    # one inlier is enough when the caller says so
    records, waiting = cluster.initialize_in_global_frame(min_inliers=1)
    assert waiting == [] and records[1].ok


def test_protocol_releases_its_device_memory(env):
    """Case (d): the library's live allocations are back at their starting values once the agents, the cluster and its
    exchange plans are gone; acceleration buffers enabled before the alignment follow X."""
    torch, L, lib, dpgo_amd = env
    gc.collect()
    n0, b0 = C.c_longlong(), C.c_longlong()
    L.check(lib.dpgo_debug_live_allocations(C.byref(n0), C.byref(b0)))
    meas, n, Ttrue, _ = _lattice(dpgo_amd)
    ranges, graphs, plan, local, agents, cluster = _team(dpgo_amd, meas, n, 4)
    for ag in agents.values():
        ag.enable_acceleration(4)
    records, waiting = cluster.initialize_in_global_frame()
    assert waiting == []
    for ag in agents.values():
        assert all(torch.equal(buf, ag.X) for buf in (ag.XPrev, ag.Y, ag.V)) and float(ag.X.abs().max()) > 0
    cluster.sweep()
    torch.cuda.synchronize()
    del cluster, agents, ag, plan, graphs, records
    gc.collect()
    n1, b1 = C.c_longlong(), C.c_longlong()
    L.check(lib.dpgo_debug_live_allocations(C.byref(n1), C.byref(b1)))
    assert (n1.value, b1.value) == (n0.value, b0.value)
