"""What the team certificate (dpgo_team_certify_device, dpgo_amd.certificate.certify_team) rests on, without a device:
(i) the agents' host data matrices assemble to the global certificate matrix, (ii) the nbr_pose map, (iii)
partition_by_ranges, (iv) the entry's refusals, (v) the symmetry probe's a-priori bound in an fp64 numpy restatement."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import certificate_cases as K
import certificate_reference as ref
from conftest import to_product_measurements


def graphs_of(meas, ranges, r, tweak=None):
    import dpgo_amd
    from dpgo_amd.agent import ExchangePlan
    from dpgo_amd.measurements import partition_by_ranges
    ranges, per_robot = partition_by_ranges(meas, ranges)
    if tweak:
        tweak(per_robot)
    graphs = []
    for a, m in enumerate(per_robot):
        pg = dpgo_amd.PoseGraph(a, r, meas.d)
        pg.setMeasurements(m)
        assert pg.n() == ranges[a][1] - ranges[a][0]
        graphs.append(pg)
    return graphs, ExchangePlan(graphs)


def team_operator(graphs, plan):
    """The operator of k_cert_apply_team's gathers as one sparse matrix: rows of robot a = [Q_aa at its own slice, its
    coupling blocks at the team tiles of its slots]; and per robot (Q_aa, C_a, nbr_pose)."""
    from dpgo_amd.certificate import team_nbr_pose
    b = graphs[0].d() + 1
    firsts, N, nbr = team_nbr_pose(plan, [g.n() for g in graphs])
    rows, pieces = [], []
    for a, g in enumerate(graphs):
        rp, ci, vals = g.quadraticMatrix()
        slots, crp, cci, cvals, G0 = g.couplingMatrix()
        assert not G0.any() and slots == plan.slots[a]
        Qa = sp.bsr_matrix((vals, ci, rp), shape=(g.n() * b, g.n() * b)).tocsr()
        Ca = sp.bsr_matrix((cvals.reshape(-1, b, b), cci, crp), shape=(g.n() * b, max(len(slots), 1) * b)).tocsr()
        team_cols = sp.bsr_matrix((cvals.reshape(-1, b, b), nbr[a][cci] if len(cci) else cci, crp), shape=(g.n() * b, N * b))
        own = sp.hstack([sp.csr_matrix((g.n() * b, firsts[a] * b)), Qa,
                         sp.csr_matrix((g.n() * b, (N - firsts[a] - g.n()) * b))])
        rows.append((own + team_cols).tocsr())
        pieces.append((Qa, Ca, nbr[a]))
    return sp.vstack(rows).tocsr(), firsts, pieces


def team_certificate_matrix(graphs, plan, X):
    """C from the agents' pieces alone: S_a = sym(Y_a^T (X_a Q_aa + G_a)_rot), G_a = X_nbr C_a^T."""
    d = graphs[0].d()
    b = d + 1
    M, firsts, pieces = team_operator(graphs, plan)
    r = X.shape[0]
    Xt = X.reshape(r, -1, b)
    lam = []
    for a, (Qa, Ca, nbr) in enumerate(pieces):
        n = graphs[a].n()
        Xa = Xt[:, firsts[a]:firsts[a] + n].reshape(r, n * b)
        Xn = Xt[:, nbr].reshape(r, len(nbr) * b) if len(nbr) else np.zeros((r, b))
        EG = np.asarray((Qa @ Xa.T).T) + np.asarray((Ca @ Xn.T).T)
        S = np.einsum("rna,rnc->nac", Xa.reshape(r, n, b)[:, :, :d], EG.reshape(r, n, b)[:, :, :d])
        Lb = np.zeros((n, b, b))
        Lb[:, :d, :d] = 0.5 * (S + S.transpose(0, 2, 1))
        lam += list(Lb)
    return (M - sp.block_diag(lam, format="csr")).tocsr()


def some_ranges(n, k, rng):
    """k uneven ranges of [0, n), one of them a single pose."""
    p = int(rng.integers(1, n - 1))
    cuts = {n - 1} if k == 2 else {p, p + 1}
    while len(cuts) < k - 1:
        cuts.add(int(rng.integers(1, n)))
    cuts = sorted(cuts)
    return [(int(a), int(b)) for a, b in zip([0] + cuts, cuts + [n])]


@pytest.mark.parametrize("d", [2, 3])
def test_agents_pieces_assemble_to_the_certificate_matrix(oracle, d):
    rng = np.random.default_rng(3 + d)
    for k in (2, 3, 4, 5):
        n = 30 + 7 * k
        om, Qb, Qs = K.random_graph(oracle, d, n, False)
        r = d + (k % 3)
        X = K.random_iterate(oracle, n, d, r, 100 + k)
        ranges = some_ranges(n, k, rng)
        assert min(e - s for s, e in ranges) == 1
        graphs, plan = graphs_of(to_product_measurements(om), ranges, r)
        Ct = team_certificate_matrix(graphs, plan, X)
        Cr = ref.certificate_matrix(Qs, X, d)
        err = ref.operator_norm1(Ct - Cr)
        print("d %d, %d robots %s: |C_team - C|_1 / |C|_1 = %.2e" % (d, k, ranges, err / ref.operator_norm1(Cr)))
        assert err <= K.SCALAR_TOL * ref.operator_norm1(Cr)


@pytest.mark.parametrize("reorder", [False, True])
def test_nbr_pose_against_a_brute_force_map(oracle, reorder):
    from dpgo_amd.agent import ExchangePlan, build_pose_graphs
    from dpgo_amd.certificate import team_nbr_pose
    from dpgo_amd.measurements import locality_order
    d, n, k = 3, 203, 4
    om, _, _ = K.random_graph(oracle, d, n, False)
    meas = to_product_measurements(om)
    ranges, graphs = build_pose_graphs(meas, n, k, 4, reorder=reorder)
    firsts, N, nbr = team_nbr_pose(ExchangePlan(graphs), [g.n() for g in graphs])
    assert N == n and firsts == [s for s, _ in ranges]
    # the team tile of caller pose g: its robot's slice, at its internal row
    where = locality_order(meas, n, k).astype(np.int64) if reorder else np.arange(n)
    for a, g in enumerate(graphs):
        if reorder:
            assert np.array_equal(firsts[a] + g.pose_order, where[ranges[a][0]:ranges[a][1]])
    robot_of = np.searchsorted([s for s, _ in ranges], np.arange(n), side="right") - 1
    want = [set() for _ in range(k)]
    for g1, g2 in zip(meas.p1, meas.p2):
        if robot_of[g1] != robot_of[g2]:
            want[robot_of[g1]].add(int(where[g2]))
            want[robot_of[g2]].add(int(where[g1]))
    for a in range(k):
        assert nbr[a].dtype == np.int32 and list(nbr[a]) == sorted(want[a])
        assert not any(firsts[a] <= j < firsts[a] + graphs[a].n() for j in nbr[a])


def test_partition_by_ranges_is_partition_contiguous_on_even_ranges(oracle):
    from dpgo_amd.measurements import partition_by_ranges, partition_contiguous
    om, _, _ = K.random_graph(oracle, 3, 203, False)
    meas = to_product_measurements(om)
    for k in (1, 2, 5, 7):
        ranges, per = partition_contiguous(meas, 203, k)
        ranges2, per2 = partition_by_ranges(meas, ranges)
        assert ranges2 == ranges
        for x, y in zip(per, per2):
            for f in ("r1", "p1", "r2", "p2", "R", "t", "kappa", "tau", "weight", "fixedWeight"):
                assert np.array_equal(getattr(x, f), getattr(y, f)), f
    for bad in ([], [(0, 100)], [(0, 100), (101, 203)], [(0, 100), (100, 100), (100, 203)], [(1, 203)]):
        with pytest.raises(ValueError):
            partition_by_ranges(meas, bad)


def test_team_entry_without_a_device_reports():
    """No HIP device: DPGO_ERR_HIP; a bad member table is an error code before any handle is touched, never an abort."""
    import dpgo_amd
    import dpgo_amd.lib as L
    if dpgo_amd.device_count() > 0:
        pytest.skip("a GPU is present (tests/test_team_certificate_gpu.py::test_team_refusals)")
    lib = L.load()
    cr = L.TeamCertifyResultC()
    x = np.zeros(64)
    fake = np.zeros(4096)  # never read: the device is looked for before any handle is
    assert lib.dpgo_team_certify_device(None, 0, L.ptr(x), None, C.byref(cr), None) == L.ERR_INVALID
    mem = (L.TeamMemberC * 2)()
    assert lib.dpgo_team_certify_device(mem, 2, L.ptr(x), None, C.byref(cr), None) == L.ERR_INVALID  # null handles
    assert b"null handle" in lib.dpgo_last_error()
    mem[0].h = mem[1].h = fake.ctypes.data
    for firsts in ((1, 2), (0, 0), (0, -1)):
        mem[0].first, mem[1].first = firsts
        assert lib.dpgo_team_certify_device(mem, 2, L.ptr(x), None, C.byref(cr), None) == L.ERR_INVALID, firsts
        assert b"tile" in lib.dpgo_last_error()
    mem[0].first, mem[1].first = 0, 3
    assert lib.dpgo_team_certify_device(mem, 2, L.ptr(x), None, C.byref(cr), None) == L.ERR_HIP
    assert lib.dpgo_team_certificate_apply_device(mem, 2, L.ptr(x), L.ptr(x), L.ptr(x)) == L.ERR_HIP
    assert lib.dpgo_team_certificate_apply_device(mem, 2, None, L.ptr(x), L.ptr(x)) == L.ERR_INVALID
    bad = L.CertifyParamsC()
    lib.dpgo_certify_params_default(C.byref(bad))
    bad.tol_rel = 0.0
    assert lib.dpgo_team_certify_device(mem, 2, L.ptr(x), C.byref(bad), C.byref(cr), None) == L.ERR_INVALID


def probe(Cm, X, W, scale):
    """symmetry_defect of include/dpgo_hip.h in fp64 numpy."""
    A, B = W @ np.asarray(Cm @ X.T), np.asarray(Cm @ W.T).T @ X.T
    return np.abs(A - B).max() / (scale * np.linalg.norm(W) * np.linalg.norm(X))


def test_symmetry_probe_bound(oracle):
    """The largest team of the GPU tests (21 x 21 x 21 lattice, 8 agents, r = 4): the rounding of a consistent team stays
    below 8 (d+1) N 2^-53; one agent's weight of one shared edge changed by 1e-3 exceeds it 100 times over."""
    from test_team_certificate_gpu import probe_bound, uneven
    c = K.F_CASES[1]
    om, Qb, Qs = K.lattice_graph(oracle, c.dims)
    n, d, r = Qb.n, om.d, c.r
    X = K.random_iterate(oracle, n, d, r, 5 + r)
    meas = to_product_measurements(om)
    t = ref.indicator(n, d) / np.sqrt(n)
    W = np.random.default_rng(1).uniform(-1, 1, (r, (d + 1) * n))
    W = np.linalg.qr((W - np.outer(W @ t, t)).T)[0].T
    scale = float(Qs.diagonal().max())
    bound = probe_bound(d, n)
    graphs, plan = graphs_of(meas, uneven(n, 8), r)
    good = probe(team_certificate_matrix(graphs, plan, X), X, W, scale)

    def heavier(per_robot):
        m = per_robot[3]
        e = int(np.nonzero(m.r1 != m.r2)[0][0])
        m.weight[e] *= 1.0 + 1e-3
    graphs, plan = graphs_of(meas, uneven(n, 8), r, tweak=heavier)
    bad = probe(team_certificate_matrix(graphs, plan, X), X, W, scale)
    print("N %d: defect %.2e (consistent), %.2e (one weight off by 1e-3), bound %.2e" % (n, good, bad, bound))
    assert good <= bound
    assert bad >= 100 * bound
