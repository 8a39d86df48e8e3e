"""GNC re-weighting on the device, kernel by kernel: the residual / weight kernel k_edge_robust (K10) and the values-only
rebuild k_rebuild_Q (K9, for Q and for the coupling blocks) against the longdouble restatement of reweighting_reference.py
within its a-priori bounds (derived there, not fitted), and every derived copy of Q -- block-Jacobi factors, symmetric
storage, its fp32 copies, the hierarchy -- after a weight change against a fresh handle built from the new values.

Each case prints its largest observed error / bound ratio (lines starting with "ratio") before it asserts."""
import ctypes as C
import os

import numpy as np
import pytest

import certificate_reference as cref
import reweighting_reference as ref
from conftest import DATA, matrix_to_tiles, tiles_to_matrix, to_product_measurements
from test_launch_geometry_gpu import DR, Handle, device_input, guard_of, library_options
from test_parity_gpu import RTOL_ELEM, _grid2d_measurements, _hierarchy_check, _random_graph, relerr

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
SYM = {"DPGO_SPLIT": "1", "DPGO_SPMM_SYMMETRIC": "1"}


def _report(case, what, ratio):
    print("ratio %-28s %-14s %.3e" % (case, what, ratio))
    return ratio


def _max_ratio(err, bound):
    """max err / bound over the entries with a positive bound; entries with a zero bound must be exact."""
    err, bound = np.asarray(err, dtype=np.float64).ravel(), np.asarray(bound, dtype=np.float64).ravel()
    assert (err[bound == 0] == 0).all(), "error where the bound is zero"
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------- the C ABI's edge entries on a geometry-suite Handle
class Edges:
    def __init__(self, h, meas, w, fixed, role=None, slot=None, check=True):
        self.h, self.m = h, len(meas.p1)
        L = h.L
        a = [L.i32(meas.p1), L.i32(meas.p2),
             None if role is None else np.ascontiguousarray(role, dtype=np.uint8), None if slot is None else L.i32(slot),
             np.ascontiguousarray(meas.R, dtype=np.float64), np.ascontiguousarray(meas.t, dtype=np.float64),
             np.ascontiguousarray(meas.kappa, dtype=np.float64), np.ascontiguousarray(meas.tau, dtype=np.float64),
             np.ascontiguousarray(w, dtype=np.float64), np.ascontiguousarray(fixed, dtype=np.uint8)]
        self.rc = h.lib.dpgo_problem_set_reweightable_edges_ex(h.h, self.m, *[L.ptr(x) for x in a])
        if check:
            L.check(self.rc)

    def reweight(self, Xd, mu, barc, w_tol=1e-8, update=True, nbr=None):
        """(return code, counts, max_rsq) of dpgo_problem_gnc_reweight_device."""
        counts, mx = (C.c_int * 3)(-1, -1, -1), C.c_double(-1.0)
        rc = self.h.lib.dpgo_problem_gnc_reweight_device(self.h.h, self.h.L.ptr(Xd), self.h.L.ptr(nbr), float(mu), float(barc),
                                                         float(w_tol), int(update), C.byref(counts), C.byref(mx))
        return rc, tuple(counts), mx.value

    def get(self):
        w, rs = np.full(max(self.m, 1), np.nan), np.full(max(self.m, 1), np.nan)
        self.h.L.check(self.h.lib.dpgo_problem_get_edge_weights(self.h.h, self.h.L.ptr(w), self.h.L.ptr(rs)))
        return w[:self.m], rs[:self.m]

    def set(self, w):
        return self.h.lib.dpgo_problem_set_edge_weights(self.h.h, self.h.L.ptr(np.ascontiguousarray(w, dtype=np.float64)))


def _q_values(h, nnzb):
    v = np.full((nnzb, h.d + 1, h.d + 1), np.nan)
    h.L.check(h.lib.dpgo_problem_get_Q_values(h.h, h.L.ptr(v)))
    return v


def _expected_counts(w, counted, w_tol):
    w = w[counted]
    out = int((w < w_tol).sum())
    inl = int(((w >= w_tol) & (w > 1.0 - w_tol)).sum())
    return (inl, out, len(w) - inl - out)


def _check_weights(case, rsq_dev, w_dev, w_before, fixed, mu, barc):
    """The weights of one update against tls_weight_fp64 on the DEVICE's rsq: 4 eps (w + mu) everywhere, exact 0.0 / 1.0
    further than 4 ulp from both thresholds; fixed edges untouched."""
    free = ~fixed
    assert np.array_equal(_bits(w_dev[fixed]), _bits(w_before[fixed])), case
    want = ref.tls_weight_fp64(rsq_dev, mu, barc)
    lower, upper = ref.tls_thresholds(mu, barc)
    r = np.sqrt(rsq_dev)
    rSq = r * r
    away = (np.abs(rSq - upper) > 4 * np.spacing(upper)) & (np.abs(rSq - lower) > 4 * np.spacing(lower))
    err = np.abs(w_dev - want)
    _report(case, "weight", _max_ratio(err[free], (4 * EPS * (want + mu))[free]))
    assert (err[free] <= 4 * EPS * (want[free] + mu)).all(), case
    sat = free & away & ((want == 0.0) | (want == 1.0))
    assert np.array_equal(_bits(w_dev[sat]), _bits(want[sat])), case


def _check_residuals(case, rsq_dev, max_rsq, meas, X, d, r, **shared):
    want, mag = ref.residuals(meas, X, **shared)
    bound = ref.rsq_bound(mag, d, r)
    err = np.abs(ref._ld(rsq_dev) - want)
    ratio = _report(case, "rsq", _max_ratio(err, bound))
    assert ratio <= 1.0, (case, ratio)
    assert _bits([max_rsq])[0] == _bits([rsq_dev.max() if len(rsq_dev) else 0.0])[0], case
    return np.asarray(want, dtype=np.float64)


def _iterates(oracle, T, d, r, seed):
    """Ground truth lifted to rank r plus 1e-3 noise (cancellation), and a random point of the manifold (O(1) residuals)."""
    n = T.shape[0]
    rng = np.random.default_rng(seed)
    return [("truth", oracle.polar_project(oracle.lift(T, r) + 1e-3 * rng.standard_normal((n, d + 1, r)), d)),
            ("random", oracle.polar_project(rng.standard_normal((n, d + 1, r)), d))]


_CACHE = {}


def _graph257(oracle, d):
    """_random_graph on 257 poses: 424 edges (two workgroups of k_edge_robust, the second ragged), a hub pose with 40
    edges in both orientations, odometry fixed and the rest free."""
    if ("g", d) not in _CACHE:
        om, T, hub = _random_graph(oracle, d, 257, 128, 40, seed=4100 + d)
        _CACHE[("g", d)] = (om, T, hub, oracle.construct_Q(257, d, om))
    return _CACHE[("g", d)]


def _w1(rng, fixed, hub_edge):
    """One third of the free edges at 0, one third in [0.05, 1], the rest at 1; then one hub edge at 1e-12."""
    w = np.ones(len(fixed))
    free = np.nonzero(~fixed)[0]
    k = len(free) // 3
    pick = rng.permutation(free)
    w[pick[:k]] = 0.0
    w[pick[k:2 * k]] = rng.uniform(0.05, 1.0, k)
    w[hub_edge] = 1e-12
    return w


def _hub_edge(om, hub):
    return int(np.nonzero(~om.fixed & ((om.p1 == hub) | (om.p2 == hub)))[0][0])


# ---------------------------------------------------------------- 2. residual and weight kernel
def _drive_edge_kernel(case, oracle, h, ed, meas, fixed, iterates, d, r, counted=None, **shared):
    """update = 0, then update = 1 at thresholds that put >= 10 % of the free edges into each branch, then the counts at
    w_tol = 0.25, per iterate."""
    guard = guard_of(d, r)
    free = ~fixed
    counted = free if counted is None else counted
    for name, X in iterates:
        tag = "%s %s" % (case, name)
        Xd = device_input(X, guard)
        w_before, _ = ed.get()
        rc, counts, mx = ed.reweight(Xd, 1.0, 1.0, update=False, **{k: v for k, v in shared.items() if k == "nbr"})
        assert rc == 0, tag
        w_same, rsq_dev = ed.get()
        assert np.array_equal(_bits(w_same), _bits(w_before)), tag  # update = 0: no weight changes
        assert counts == _expected_counts(w_before, counted, 1e-8), tag  # ... the counts describe the stored weights
        href = {k: (v.cpu().numpy().reshape(-1, d + 1, r) if k == "nbr" else v) for k, v in shared.items()}
        rsq_ref = _check_residuals(tag, rsq_dev, mx, meas, X, d, r, **href)
        if free.sum() >= 10:
            mu, barc = ref.tls_parameters_for(rsq_ref[free])
            share = np.bincount(ref.tls_branches(rsq_ref[free], mu, barc), minlength=3) / float(free.sum())
            assert (share >= 0.1).all(), (tag, share)
        else:
            mu, barc = 0.7, float(np.sqrt(max(rsq_ref.max(), 1e-30)))
        rc, counts, mx = ed.reweight(Xd, mu, barc, update=True, **{k: v for k, v in shared.items() if k == "nbr"})
        assert rc == 0, tag
        w_dev, rsq2 = ed.get()
        assert np.array_equal(_bits(rsq2), _bits(rsq_dev)) and _bits([mx])[0] == _bits([rsq_dev.max()])[0], tag
        _check_weights(tag, rsq_dev, w_dev, w_before, fixed, mu, barc)
        assert counts == _expected_counts(w_dev, counted, 1e-8), (tag, counts)
        rc, counts, _ = ed.reweight(Xd, mu, barc, w_tol=0.25, update=False, **{k: v for k, v in shared.items() if k == "nbr"})
        want = _expected_counts(w_dev, counted, 0.25)
        assert rc == 0 and counts == want, (tag, counts, want)
        if free.sum() >= 10:
            assert min(want) > 0, (tag, want)  # both tails and "undecided" are populated
        assert np.array_equal(_bits(ed.get()[0]), _bits(w_dev)), tag


@pytest.mark.parametrize("d,r", DR)
def test_edge_residuals_and_tls_weights_match_longdouble(oracle, d, r):
    """k_edge_robust<d, r> through dpgo_problem_gnc_reweight_device on 257 poses / 424 edges, on a single edge and on an
    empty registration: rsq of every edge (fixed ones too) within c_rsq u mag of the longdouble residual, max_rsq bitwise
    the largest device rsq, the weights of the three GNC-TLS branches from the device's own rsq, fixed weights kept
    bitwise, integer counts at w_tol = 1e-8 and 0.25, nothing changed by update = 0; the exactly representable threshold
    case and the argument checks."""
    om, T, hub, Qb = _graph257(oracle, d)
    with library_options({}) as lib:
        h = Handle(lib, Qb, r, d)
        try:
            ed = Edges(h, om, np.ones(om.m), om.fixed)
            assert om.m > 256 and om.m % 256 != 0 and (om.p2 < om.p1).any() and om.fixed.any() and (~om.fixed).any()
            _drive_edge_kernel("d%d r%d n257" % (d, r), oracle, h, ed, om, om.fixed.copy(), _iterates(oracle, T, d, r, 7 + r), d, r)
            # argument checks: nothing is launched, the stored weights and residuals stay
            w_now, rsq_now = ed.get()
            Xd = device_input(_iterates(oracle, T, d, r, 1)[1][1], guard_of(d, r))
            for mu in (0.0, -1.0, float("nan")):
                assert ed.reweight(Xd, mu, 1.0, update=True)[0] == h.L.ERR_INVALID
            assert ed.reweight(None, 1.0, 1.0)[0] == h.L.ERR_INVALID
            w_after, rsq_after = ed.get()
            assert np.array_equal(_bits(w_after), _bits(w_now)) and np.array_equal(_bits(rsq_after), _bits(rsq_now))
            # an empty registration: the entry succeeds and counts nothing
            empty = Edges(h, om.subset([]), np.zeros(0), np.zeros(0, dtype=bool))
            rc, counts, mx = empty.reweight(Xd, 1.0, 1.0, update=True)
            assert (rc, counts, mx) == (0, (0, 0, 0), 0.0)
            rc, counts, mx = empty.reweight(Xd, 1.0, 1.0, update=False)
            assert (rc, counts, mx) == (0, (0, 0, 0), 0.0)
        finally:
            h.close()
        # m = 1: the two-pose graph's only edge, registered free
        om2, T2, _ = _random_graph(oracle, d, 2, 0, 0, seed=4200 + d)
        h = Handle(lib, oracle.construct_Q(2, d, om2), r, d)
        try:
            fixed1 = np.zeros(1, dtype=bool)
            ed = Edges(h, om2, np.ones(1), fixed1)
            _drive_edge_kernel("d%d r%d m1" % (d, r), oracle, h, ed, om2, fixed1, _iterates(oracle, T2, d, r, 3), d, r)
            # integer data: identity rotations, t = 0, p_j - p_i = (3, 0, ..), tau = 1: rSq0 = 9 exactly = upper at
            # mu = 1/8, barc = 1 -> weight 0.0; further exact cases: whatever the oracle returns in fp64
            z = np.zeros(1, dtype=np.int64)
            exact = oracle.Measurements(d, z, z.copy(), z.copy(), z + 1, np.eye(d)[None], np.zeros((1, d)), np.ones(1),
                                        np.ones(1), np.ones(1), fixed1)
            ed = Edges(h, exact, np.ones(1), fixed1)
            X = np.zeros((2, d + 1, r))
            X[:, :d, :d] = np.eye(d)
            X[1, d, 0] = 3.0
            Xd = device_input(X, guard_of(d, r))
            for mu, barc in [(0.125, 1.0), (8.0, 1.0), (1.0, 3.0), (1.0, 5.0), (0.5, 3.0), (2.0, 2.0), (0.125, 9.0)]:
                assert ed.set(np.ones(1)) == 0
                rc, counts, mx = ed.reweight(Xd, mu, barc, update=True)
                w, rsq = ed.get()
                want = float(oracle.gnc_tls_weight(np.array([3.0]), mu, barc)[0])
                assert rc == 0 and rsq[0] == 9.0 and mx == 9.0, (mu, barc, rsq)
                if 0.0 < want < 1.0:
                    assert abs(w[0] - want) <= 4 * EPS * (want + mu), (mu, barc, w, want)
                else:
                    assert _bits(w)[0] == _bits([want])[0], (mu, barc, w, want)
                assert counts == _expected_counts(w, ~fixed1, 1e-8)
                if (mu, barc) == (0.125, 1.0):
                    assert ref.tls_thresholds(mu, barc)[1] == 9.0 and w[0] == 0.0 and counts == (0, 1, 0)
        finally:
            h.close()


@pytest.mark.parametrize("d,r", [(3, 5), (2, 2)])
def test_nan_pose_keeps_the_weights_of_its_edges_and_Q_finite(oracle, d, r):
    """One pose's translation row is NaN in an otherwise random iterate (257 poses / 424 edges): the residuals of its edges
    are NaN, no GNC-TLS weight can be computed for them, and dpgo_problem_gnc_reweight_device(update = 1) does not store
    one -- those edges keep their weights bitwise and are counted as undecided, so that the three counts still sum to the
    number of free edges; every other free edge gets its weight as usual, max_rsq is the largest finite residual, and
    the rebuilt Q is finite everywhere."""
    om, T, hub, Qb = _graph257(oracle, d)
    fixed = om.fixed.copy()
    free = ~fixed
    degree = np.bincount(np.r_[om.p1[free], om.p2[free]], minlength=257)
    pose = int(next(i for i in range(257) if i != hub and degree[i] >= 2))
    at_pose = (om.p1 == pose) | (om.p2 == pose)
    assert (free & at_pose).sum() >= 2 and (fixed & at_pose).any() and (free & ~at_pose).sum() >= 10
    X = _iterates(oracle, T, d, r, 7 + r)[1][1].copy()
    rsq_ref = np.asarray(ref.residuals(om, X)[0], dtype=np.float64)  # (the edges away from the pose do not see the NaN)
    mu, barc = ref.tls_parameters_for(rsq_ref[free & ~at_pose])
    X[pose, d, :] = np.nan
    w0 = np.where(fixed, 1.0, np.random.default_rng(90 + d).uniform(0.2, 0.9, om.m))
    tag = "d%d r%d nan pose" % (d, r)
    with library_options({}) as lib:
        h = Handle(lib, Qb, r, d)
        try:
            ed = Edges(h, om, np.ones(om.m), fixed)
            assert ed.set(w0) == 0
            rc, counts, mx = ed.reweight(device_input(X, guard_of(d, r)), mu, barc, update=True)
            assert rc == 0, tag
            w_dev, rsq_dev = ed.get()
            assert np.array_equal(np.isnan(rsq_dev), at_pose) and np.isfinite(rsq_dev[~at_pose]).all(), tag
            assert sum(counts) == int(free.sum()), (tag, counts)
            assert np.array_equal(_bits(w_dev[at_pose]), _bits(w0[at_pose])), tag
            away = ~at_pose
            _check_weights(tag, rsq_dev[away], w_dev[away], w0[away], fixed[away], mu, barc)
            inl, out, und = _expected_counts(w_dev, free & away, 1e-8)
            assert counts == (inl, out, und + int((free & at_pose).sum())), (tag, counts)
            assert _bits([mx])[0] == _bits([np.nanmax(rsq_dev)])[0], tag
            assert np.isfinite(_q_values(h, Qb.nnzb)).all(), tag
        finally:
            h.close()


def _agent_problem(oracle, name, a, robots=3):
    """One agent's block of a three-robot split through PoseGraph, with the G coupling and every edge registered."""
    import dpgo_amd
    if name == "smallGrid3D":
        dataset, n = dpgo_amd.read_g2o_file(os.path.join(DATA, "smallGrid3D.g2o"))
        r = 5
    else:
        om, _, _ = _random_graph(oracle, 2, 90, 60, 20, seed=4300)
        dataset, n, r = to_product_measurements(om), 90, 3
    d = dataset.d
    ranges, per = dpgo_amd.partition_contiguous(dataset, n, robots)
    pg = dpgo_amd.PoseGraph(a, r, d)
    pg.setMeasurements(per[a])
    prob = dpgo_amd.QuadraticProblem(pg, host_linear_term=False)
    slots = prob.setCouplingFromPoseGraph()
    assert prob.setReweightableEdges(include_shared=True) == len(pg.measurements())
    meas = pg.measurements()
    role, slot, slots_ref = ref.roles_and_slots(meas, a)
    assert slots_ref == [tuple(s) for s in slots]
    fixed = np.asarray(meas.fixedWeight, dtype=bool) | pg.odometry_mask(meas)
    return pg, prob, meas, role, slot, slots, fixed, d, r


@pytest.mark.parametrize("name", ["smallGrid3D", "random2D"])
def test_shared_edges_take_the_neighbour_tiles(oracle, name):
    """Roles 1 and 2 at a random iterate: the middle agent of a three-robot split (outgoing and incoming shared edges),
    registered through setCouplingFromPoseGraph + setReweightableEdges(include_shared=True), neighbour tiles = random
    manifold points.  rsq, weights and counts as for private edges; an incoming shared edge (role 2) is not counted;
    without the neighbour tiles the entry is refused, and so is the host flavour."""
    import torch
    a = 1
    pg, prob, meas, role, slot, slots, fixed, d, r = _agent_problem(oracle, name, a)
    assert (role == 1).any() and (role == 2).any() and (role == 0).any()
    assert (~fixed & (role == 2)).any() and (~fixed & (role == 1)).any()
    na = pg.n()
    rng = np.random.default_rng(17)
    nbr = torch.from_numpy(oracle.polar_project(rng.standard_normal((len(slots), d + 1, r)), d)).to("cuda")
    torch.cuda.synchronize()

    class View:  # the wrapper's handle behind the Handle interface Edges drives
        pass
    h = View()
    import dpgo_amd.lib as L
    h.lib, h.L, h.h, h.d, h.r, h.n = prob._lib, L, prob.handle, d, r, na
    ed = Edges.__new__(Edges)
    ed.h, ed.m = h, len(meas)
    X = oracle.polar_project(rng.standard_normal((na, d + 1, r)), d)
    Xd = device_input(X, guard_of(d, r))
    assert ed.reweight(Xd, 1.0, 1.0, update=True, nbr=None)[0] == L.ERR_INVALID  # shared edges need the tiles
    counts, mx = (C.c_int * 3)(), C.c_double()
    assert prob._lib.dpgo_problem_gnc_reweight(prob.handle, L.ptr(np.ascontiguousarray(X)), 1.0, 1.0, 1e-8, 1, C.byref(counts),
                                               C.byref(mx)) == L.ERR_STATE
    its = [("random", X), ("random2", oracle.polar_project(rng.standard_normal((na, d + 1, r)), d))]
    _drive_edge_kernel("%s agent%d" % (name, a), oracle, h, ed, meas, fixed, its, d, r, counted=~fixed & (role != 2),
                       nbr=nbr, role=role, slot=slot)


# ---------------------------------------------------------------- 3. values-only rebuild
def _check_product(case, h, rowptr, colidx, vals_ld, E, V, Vd, guard):
    want = ref.block_product(rowptr, colidx, vals_ld, V)
    got = h.spmm_device(Vd, guard)
    ratio = _report(case, "Q(w1) V", ref.fro(ref._ld(got) - want) / ref.product_bound(rowptr, colidx, E, V, want))
    assert ratio <= 1.0, (case, ratio)
    return got


def _storage_in_use(h):
    v = C.c_int(-1)
    h.L.check(h.lib.dpgo_problem_set_spmm_variant(h.h, 0, C.byref(v)))
    return {1: "plain", 2: "symmetric"}[v.value]


def _rebuild_case(case, oracle, lib, om, hub_edge, Qb0, w0, d, r, storage, seed, values=True):
    """set_edge_weights(w1) on a handle registered at w0: values and product against longdouble, w1 -> w2 -> w1 bitwise,
    update_Q_values recomputes the base, a new pattern drops the registration."""
    n = Qb0.n
    rng = np.random.default_rng(seed)
    guard = guard_of(d, r)
    fixed = om.fixed.copy()
    w1 = _w1(rng, fixed, hub_edge)
    w2 = np.where(fixed, 1.0, rng.uniform(0.0, 1.0, om.m))
    V = rng.standard_normal((n, d + 1, r))
    Vd = device_input(V, guard)
    h = Handle(lib, Qb0, r, d)
    try:
        ed = Edges(h, om, w0, fixed)
        assert _storage_in_use(h) == storage, case
        first = h.spmm_device(Vd, guard)  # (every copy of Q exists before the weights change)
        assert relerr(first, (Qb0.to_scipy().tocsr() @ V.reshape(-1, r)).reshape(V.shape)) < 1e-13, case
        assert ed.set(w1) == 0
        assert _storage_in_use(h) == storage, case
        want, M, count = ref.rebuilt_Q(Qb0.rowptr, Qb0.colidx, Qb0.vals, om, w0, w1)
        E = ref.value_bound(M, count, d)
        vals1 = _q_values(h, Qb0.nnzb)
        ratio = _report(case, "Q values", _max_ratio(np.abs(ref._ld(vals1) - want), E))
        assert ratio <= 1.0, (case, ratio)
        p1 = _check_product(case, h, Qb0.rowptr, Qb0.colidx, want, E, V, Vd, guard)
        # idempotence without drift: the rebuild starts from q_base and sums in a fixed order
        assert ed.set(w2) == 0
        p2 = h.spmm_device(Vd, guard)
        assert not np.array_equal(p2, p1), case
        assert ed.set(w1) == 0
        assert np.array_equal(_bits(h.spmm_device(Vd, guard)), _bits(p1)), case
        assert np.array_equal(_bits(_q_values(h, Qb0.nnzb)), _bits(vals1)), case
        assert np.array_equal(_bits(ed.get()[0]), _bits(w1)), case
        # update_Q_values with 1.5 x the current values (weights w2 registered): the base is recomputed, so that
        # set_edge_weights(w1) gives 1.5 Q(w2) - contrib(w2) + contrib(w1)
        assert ed.set(w2) == 0
        vals2 = _q_values(h, Qb0.nnzb)
        scaled = np.ascontiguousarray(1.5 * vals2)
        h.L.check(h.lib.dpgo_problem_update_Q_values(h.h, h.L.ptr(scaled)))
        assert relerr(h.spmm_device(Vd, guard), 1.5 * p2) < 1e-13, case
        assert ed.set(w1) == 0
        want, M, count = ref.rebuilt_Q(Qb0.rowptr, Qb0.colidx, scaled, om, w2, w1)
        E = ref.value_bound(M, count, d)
        ratio = _report(case, "values 1.5x", _max_ratio(np.abs(ref._ld(_q_values(h, Qb0.nnzb)) - want), E))
        assert ratio <= 1.0, (case, ratio)
        _check_product(case + " 1.5x", h, Qb0.rowptr, Qb0.colidx, want, E, V, Vd, guard)
        # a new pattern drops the registration
        Qn = oracle.construct_Q(n, d, om.subset(np.arange(om.m - 1)))
        assert Qn.nnzb != Qb0.nnzb
        h.L.check(h.lib.dpgo_problem_set_Q_bsr(h.h, Qn.nnzb, h.L.ptr(Qn.rowptr), h.L.ptr(Qn.colidx), h.L.ptr(Qn.vals)))
        assert ed.set(w1) == h.L.ERR_STATE, case
        assert h.lib.dpgo_problem_get_edge_weights(h.h, h.L.ptr(np.zeros(om.m)), None) == h.L.ERR_STATE, case
    finally:
        h.close()


@pytest.mark.parametrize("d,r", DR)
def test_values_only_rebuild_matches_longdouble(oracle, d, r):
    """dpgo_problem_set_edge_weights on 257 poses (hub slot with 40 contributions, one hub edge at 1e-12), registered at
    weights in [0.2, 1]: on the plain and on the symmetric storage of Q."""
    om, T, hub, _ = _graph257(oracle, d)
    rng = np.random.default_rng(50 + d)
    w0 = np.where(om.fixed, 1.0, rng.uniform(0.2, 1.0, om.m))
    om0 = om.subset(np.arange(om.m))
    om0.weight = w0.copy()
    Qb0 = oracle.construct_Q(257, d, om0)
    for storage, env in (("plain", {}), ("symmetric", SYM)):
        with library_options(env) as lib:
            _rebuild_case("d%d r%d %s" % (d, r, storage), oracle, lib, om, _hub_edge(om, hub), Qb0, w0, d, r, storage, seed=60 + r)


def test_grid_370x370_runs_every_trip_of_the_grid_stride_loops(oracle):
    """273 060 edges and 683 020 blocks on 136 900 poses (d = r = 2): the launch cap holds 262 144 lanes, so k_edge_robust
    takes a second trip of its grid-stride loop and k_rebuild_Q a third; residuals, weights, counts, rebuilt values and
    the product as on the small graphs."""
    d = r = 2
    om, n = _grid2d_measurements(oracle, 370, 370, seed=9)
    assert om.m == 273060 > 262144 and n + 2 * om.m > 2 * 262144
    om.fixed = om.p1 + 1 == om.p2
    Qb = oracle.construct_Q(n, d, om)
    rng = np.random.default_rng(2)
    X = oracle.polar_project(rng.standard_normal((n, d + 1, r)), d)
    with library_options({}) as lib:
        h = Handle(lib, Qb, r, d)
        try:
            ed = Edges(h, om, np.ones(om.m), om.fixed)
            _drive_edge_kernel("grid370", oracle, h, ed, om, om.fixed.copy(), [("random", X)], d, r)
            w0, _ = ed.get()  # what the update left: the registered weights of the rebuild below
            vals0 = _q_values(h, Qb.nnzb)
            w1 = _w1(rng, om.fixed, int(np.nonzero(~om.fixed)[0][-1]))  # (the last edge: third trip of the rebuild)
            assert ed.set(w1) == 0
            want, M, count = ref.rebuilt_Q(Qb.rowptr, Qb.colidx, vals0, om, w0, w1)
            E = ref.value_bound(M, count, d)
            ratio = _report("grid370", "Q values", _max_ratio(np.abs(ref._ld(_q_values(h, Qb.nnzb)) - want), E))
            assert ratio <= 1.0, ratio
            guard = guard_of(d, r)
            V = rng.standard_normal((n, d + 1, r))
            _check_product("grid370", h, Qb.rowptr, Qb.colidx, want, E, V, device_input(V, guard), guard)
        finally:
            h.close()


@pytest.mark.parametrize("name", ["smallGrid3D", "random2D"])
def test_shared_edges_rebuild_the_coupling_blocks(oracle, name):
    """K9 on the coupling blocks: after set_edge_weights(w1) G is unchanged until
    dpgo_problem_update_G_from_neighbors_device, then G = C(w1) * neighbour tiles and euc_grad(X) = Q(w1) X + G(w1)
    against longdouble within the product bounds."""
    import torch
    a = 1
    pg, prob, meas, role, slot, slots, fixed, d, r = _agent_problem(oracle, name, a)
    na = pg.n()
    rng = np.random.default_rng(23)
    w0 = np.asarray(meas.weight, dtype=np.float64).copy()
    free = np.nonzero(~fixed)[0]
    w1 = _w1(rng, fixed, int(free[np.nonzero(role[free] != 0)[0][0]]))
    nbr_h = oracle.polar_project(rng.standard_normal((len(slots), d + 1, r)), d)
    nbr = torch.from_numpy(nbr_h).to("cuda")
    X = oracle.polar_project(rng.standard_normal((na, d + 1, r)), d)
    zero = torch.zeros((na, d + 1, r), dtype=torch.float64, device="cuda")
    out = torch.empty_like(zero)
    torch.cuda.synchronize()

    def G_now():
        prob.spmmDevice(zero, out, add_G=True)  # Q 0 + G
        torch.cuda.synchronize()
        return out.cpu().numpy().copy()

    prob.updateLinearMatrixFromNeighbors(nbr)
    G0 = G_now()
    assert np.abs(G0).max() > 0
    prob.setEdgeWeights(w1)
    assert np.array_equal(_bits(G_now()), _bits(G0))  # refresh_after_weights: G follows at the next update_G call
    prob.updateLinearMatrixFromNeighbors(nbr)
    G1 = G_now()
    _, crow, ccol, cvals, G0lin = pg.couplingMatrix()
    assert not np.any(G0lin)
    C1, Mc, cc = ref.rebuilt_C(crow, ccol, len(slots), cvals, meas, w0, w1, role, slot)
    Gw = ref.block_product(crow, ccol, C1, nbr_h)
    bG = ref.product_bound(crow, ccol, ref.value_bound(Mc, cc, d), nbr_h, Gw)
    ratio = _report(name, "G(w1)", ref.fro(ref._ld(G1) - Gw) / bG)
    assert ratio <= 1.0, ratio
    qrow, qcol, qvals = pg.quadraticMatrix()
    Q1, Mq, cq = ref.rebuilt_Q(qrow, qcol, qvals, meas, w0, w1, role)
    QX = ref.block_product(qrow, qcol, Q1, X)
    bQ = ref.product_bound(qrow, qcol, ref.value_bound(Mq, cq, d), X, QX)
    eg = matrix_to_tiles(prob.EucGrad(tiles_to_matrix(X)), d)
    ratio = _report(name, "euc_grad", ref.fro(ref._ld(eg) - (QX + Gw)) / (bQ + bG))
    assert ratio <= 1.0, ratio
    # and the oracle's own construction at the new weights says the same
    om1 = oracle.Measurements(d, meas.r1, meas.p1, meas.r2, meas.p2, meas.R, meas.t, meas.kappa, meas.tau, w1, fixed)
    Go = oracle.construct_G(na, d, r, om1.subset(np.nonzero(role != 0)[0]), a, {tuple(s): nbr_h[k] for k, s in enumerate(slots)})
    assert relerr(G1, Go) < 1e-12


# ---------------------------------------------------------------- 4. every derived copy follows the weights
PATHS = {  # name: (library switches, one-launch solve, preconditioner)
    "plain-jacobi": ({}, False, "jacobi"),
    "one-launch-jacobi": ({}, True, "jacobi"),
    "one-launch-additive": ({}, True, "additive"),
    "symmetric-jacobi": (SYM, False, "jacobi"),
    "symmetric-multilevel-fp32": (SYM, False, "multilevel"),
    "symmetric-multilevel-fp64": (dict(SYM, DPGO_ML_OPERATOR_BITS="64"), False, "multilevel"),
    "plain-multilevel": ({}, False, "multilevel"),
}


# Parameters of every solve of section 4.  Two outer iterations: the fewest with which each path runs its own solve (the
# one-launch kernel is not selected for RTR_iterations = 1, solve.hip).  Ten tCG steps per outer iteration: a stale copy
# changes tCG from its first step, while the comparison with a handle built from the host's values must itself be well
# posed -- K9's two-step rebuild and the host construction differ in the last bit of Q's values, and with block-Jacobi
# on this w1 the ORACLE's own solve answers a one-ulp perturbation of Q(w1) with 1.4e-9 in the cost at the default 50
# steps (3.5e-9 at three outer iterations), above the 1e-10 the comparison asserts, against 5e-14 at ten.
# tests/test_reweighting_reference_cpu.py holds the oracle to a hundredth of both tolerances at these parameters.
RTR_ITERATIONS, RTR_TCG_ITERATIONS = 2, 10


def _set_w1(om):
    """The w1 of section 4: _w1 on the loop closures, the first of them at 1e-12."""
    return _w1(np.random.default_rng(31), om.fixed, int(np.nonzero(~om.fixed)[0][0]))


def _workload(oracle, dim):
    """(measurements, n, r, chordal start): 12 x 12 x 9 grid at r = 5, or the 36 x 36 lattice at r = 3; loop closures free,
    odometry fixed."""
    if ("w", dim) not in _CACHE:
        if dim == 3:
            om, n, _ = oracle.synthetic_grid(12, 12, 9, seed=0)
            r = 5
        else:
            om, n = _grid2d_measurements(oracle, 36, 36, seed=5)
            om.fixed = om.p1 + 1 == om.p2
            r = 3
        assert n == 1296
        X0 = np.ascontiguousarray(oracle.lift(oracle.chordal_initialization(om, n), r))
        _CACHE[("w", dim)] = (om, n, r, X0)
    return _CACHE[("w", dim)]


def _problem(oracle, om, n, r, persistent, Q=None):
    import dpgo_amd
    pg = dpgo_amd.PoseGraph(0, r, om.d)
    pg.setMeasurements(to_product_measurements(om))
    assert pg.n() == n
    if Q is not None:  # the handle takes these values (oracle.construct_Q), not the wrapper's own construction
        rp, ci, _ = pg.quadraticMatrix()
        assert np.array_equal(rp, Q.rowptr) and np.array_equal(ci, Q.colidx)
        pg._Q = (Q.rowptr, Q.colidx, np.ascontiguousarray(Q.vals))
    prob = dpgo_amd.QuadraticProblem(pg)
    prob.setPersistent(persistent)
    return pg, prob


def _solve(prob, precond, X0, rtr):
    import torch
    import dpgo_amd
    opt = dpgo_amd.QuadraticOptimizer(prob, dpgo_amd.ROptParameters(precond=precond, RTR_iterations=rtr,
                                                                     RTR_tCG_iterations=RTR_TCG_ITERATIONS))
    Xd = torch.from_numpy(X0.copy()).to("cuda")
    torch.cuda.synchronize()
    res = opt.optimizeDevice(Xd)
    torch.cuda.synchronize()
    return res, Xd.cpu().numpy()


def _assert_path(path, prob, res):
    env, persistent, precond = PATHS[path]
    assert res.precond_used == precond, (path, res.precond_used)
    assert (prob.persistentInfo()["last_members"] > 0) == persistent, (path, prob.persistentInfo())
    if env.get("DPGO_SPMM_SYMMETRIC") == "1":
        assert prob.setSpmmVariant("auto") == "symmetric", path
        if not persistent:
            assert prob.tcgKernelInfo()["symmetric"], path
    if precond == "multilevel":
        assert len(prob.multilevelInfo()["sizes"]) == 2, path  # a two-level cycle
    if path == "symmetric-multilevel-fp32":  # the cycle streamed the fp32 copies, or this case has not reached them
        bits = prob.multilevelOperatorBits()
        assert bits["bits"] == 32 and bits["active"], (path, bits)
    if path == "symmetric-multilevel-fp64":
        bits = prob.multilevelOperatorBits()
        assert bits["bits"] == 64 and not bits["active"], (path, bits)


def _evaluations_follow(oracle, path, prob, Q1, X, d, r):
    """Every evaluation entry of the warm handle against the oracle problem on Q(w1), at the geometry suite's
    tolerances."""
    import torch
    precond = PATHS[path][2]
    n = Q1.n
    op = oracle.QuadraticProblem(Q1, None, r, d, precond="jacobi")
    V = np.random.default_rng(8).standard_normal(X.shape)
    Vt = oracle.tangent_project(X, V, d)
    Xm, Vm, Vtm = tiles_to_matrix(X), tiles_to_matrix(V), tiles_to_matrix(Vt)
    fo, gn = op.f(X), op.rie_grad_norm(X)
    assert abs(prob.f(Xm) - fo) <= 1e-12 * abs(fo), path
    assert relerr(matrix_to_tiles(prob.EucGrad(Xm), d), op.euc_grad(X)) < RTOL_ELEM, path
    assert relerr(matrix_to_tiles(prob.EucHessianEta(Xm, Vm), d), op.euc_hess(V)) < 1e-13, path
    S = op.sym_ytg(X, op.euc_grad(X))
    assert relerr(matrix_to_tiles(prob.RieHessianEta(Xm, Vtm), d), op.rie_hess(X, S, Vt)) < RTOL_ELEM, path
    Xd = torch.from_numpy(np.ascontiguousarray(X)).to("cuda")
    torch.cuda.synchronize()
    xqx, xg, g2 = prob.evalTermsDevice(Xd)
    assert abs(xqx - 2 * fo) <= 1e-12 * abs(2 * fo) and xg == 0.0 and abs(g2 - gn * gn) <= 1e-12 * gn * gn, path
    assert relerr(matrix_to_tiles(prob.PreConditioner(Xm, Vm, precond="jacobi"), d), op.precondition(X, V)) < RTOL_ELEM, path
    want = cref.certificate_apply(cref.sparse_Q(Q1), Xm, Vm, d)
    assert np.linalg.norm(prob.certificateApply(Xm, Vm) - want) <= 1e-12 * np.linalg.norm(want), path
    if precond == "multilevel":
        Z = matrix_to_tiles(prob.PreConditioner(Xm, Vtm, precond="multilevel"), d)
        opm = oracle.QuadraticProblem(Q1, None, r, d, precond="amg", amg_k=prob.multilevelInfo()["ks"])
        _hierarchy_check(oracle, prob, opm)
        assert relerr(Z, opm.precondition(X, Vt)) < 1e-9, path


def _compare(oracle, path, dim, change, rtr):
    """The figures of one warm-against-fresh comparison (the path and evaluation assertions are made on the way)."""
    env, persistent, precond = PATHS[path]
    om, n, r, X0 = _workload(oracle, dim)
    d = om.d
    free = np.nonzero(~om.fixed)[0]
    with library_options(env):
        pg, prob = _problem(oracle, om, n, r, persistent)
        res0, _ = _solve(prob, precond, X0, rtr)  # every copy exists and is current
        _assert_path(path, prob, res0)
        assert prob.setReweightableEdges() == om.m
        if change == "set":
            w1 = _set_w1(om)
            prob.setEdgeWeights(w1)
        else:  # the same through the residual kernel: thresholds at the 30 % / 70 % quantiles of the start's residuals
            import torch
            rsq = np.asarray(ref.residuals(om, X0)[0], dtype=np.float64)
            mu, barc = ref.tls_parameters_for(rsq[free])
            Xd = torch.from_numpy(X0.copy()).to("cuda")
            torch.cuda.synchronize()
            counts, _ = prob.gncReweightDevice(Xd, None, mu, barc, update=True)
            w1, _ = prob.getEdgeWeights()
            assert min(counts) >= 0.1 * len(free) and sum(counts) == len(free), counts
            assert (w1[om.fixed] == 1.0).all()
        assert (w1[free] == 0.0).sum() >= len(free) // 4
        om1 = om.subset(np.arange(om.m))
        om1.weight = np.asarray(w1, dtype=np.float64).copy()
        Q1 = oracle.construct_Q(n, d, om1)
        warm_vals = np.full(Q1.vals.shape, np.nan)
        import dpgo_amd.lib as L
        L.check(prob._lib.dpgo_problem_get_Q_values(prob.handle, L.ptr(warm_vals)))
        _evaluations_follow(oracle, path, prob, Q1, X0, d, r)
        res_w, X_w = _solve(prob, precond, X0, rtr)
        _assert_path(path, prob, res_w)
        pg2, fresh = _problem(oracle, om1, n, r, persistent, Q=Q1)
        res_f, X_f = _solve(fresh, precond, X0, rtr)
        _assert_path(path, fresh, res_f)
        # ... and a fresh handle given the warm handle's own values of Q: the same input, bit for bit
        pg3, twin = _problem(oracle, om1, n, r, persistent, Q=oracle.BSR(n, d + 1, Q1.rowptr, Q1.colidx, warm_vals))
        res_t, X_t = _solve(twin, precond, X0, rtr)
    counts = lambda res: (res.tcg_iterations, res.rtr_iterations, res.precond_used)  # noqa: E731
    fig = dict(path=path, change=change, rtr=rtr, first=counts(res0), warm=counts(res_w), fresh=counts(res_f), twin=counts(res_t),
               relerr=relerr(X_w, X_f), cost=abs(res_w.fOpt - res_f.fOpt) / abs(res_f.fOpt),
               cost0=abs(res_w.fInit - res_f.fInit) / abs(res_f.fInit),
               bitwise=bool(np.array_equal(_bits(X_w), _bits(X_t)) and res_w.fOpt == res_t.fOpt),
               values=relerr(warm_vals, Q1.vals))
    print("solve", fig)
    return fig


def _warm_against_fresh(oracle, path, dim, change):
    """The comparison with a fresh handle (built from oracle.construct_Q(w1): counts, iterate 1e-7, cost 1e-10), then the
    same against a fresh handle that is given the warm handle's own values of Q: there nothing differs in the input, so
    nothing may differ in the output -- one bit would mean a copy that did not follow."""
    fig = _compare(oracle, path, dim, change, RTR_ITERATIONS)
    assert fig["twin"] == fig["warm"] and fig["bitwise"], fig
    assert fig["warm"] == fig["fresh"], fig  # tCG / RTR counts, precond_used
    assert fig["relerr"] < 1e-7, fig
    assert fig["cost"] <= 1e-10 and fig["cost0"] <= 1e-10, fig


@pytest.mark.parametrize("path", [p for p in PATHS if p != "plain-multilevel"])
def test_every_copy_of_Q_follows_set_edge_weights(oracle, path):
    """3-D grid of 1 296 poses at r = 5: a handle that solved at the registered weights, so that its block-Jacobi factors,
    symmetric storage, fp32 copies and hierarchy exist, then takes set_edge_weights(w1) and solves again from the same
    start -- as a fresh handle built from oracle.construct_Q(w1) does: same tCG / RTR counts and preconditioner, iterate
    to 1e-7, cost to 1e-10; before that solve every evaluation entry matches the oracle on Q(w1).

    Measured (rel. difference of the iterate / of the cost, warm against fresh; 17 tCG steps on the block-Jacobi paths):
    plain-jacobi 1.8e-15 / 4.5e-14, one-launch-jacobi 2.8e-15 / 3.6e-14, symmetric-jacobi 1.7e-15 / 6.4e-14,
    one-launch-additive 5.8e-13 / 4.6e-14, symmetric-multilevel 2.5e-13 / 4.5e-14 (fp32 copies) and 2.2e-13 / 4.5e-14;
    the rebuilt values of Q differ from the host's by 7e-17.  At the library's default of 50 tCG steps per outer iteration
    the block-Jacobi paths gave 9.5e-9 / 1.4e-10 (plain), 9.0e-9 / 3.4e-10 (one launch) and 4.0e-9 / 1.0e-11 (symmetric),
    as much as the oracle's own solve moves under a one-ulp perturbation of Q(w1) (RTR_TCG_ITERATIONS above)."""
    _warm_against_fresh(oracle, path, 3, "set")


@pytest.mark.parametrize("path", ["plain-jacobi", "symmetric-multilevel-fp32"])
def test_every_copy_of_Q_follows_gnc_reweight_device(oracle, path):
    """The same with the weights changed by gncReweightDevice(update=True)."""
    _warm_against_fresh(oracle, path, 3, "gnc")


def test_v_cycle_follows_set_edge_weights_in_2d(oracle):
    """The 2-D counterpart (36 x 36 lattice, r = 3) on the V-cycle path."""
    _warm_against_fresh(oracle, "plain-multilevel", 2, "set")
