"""Robust costs on the device: k_edge_robust / k_edge_robust_finish through dpgo_problem_robust_reweight_device, its Python
and distributed drivers, against the longdouble restatement of robust_cost_reference.py within its a-priori bounds (derived
there, not fitted).

Each case prints its largest observed error / bound ratio (lines starting with "ratio") before it asserts."""
import ctypes as C
import os

import numpy as np
import pytest

import reweighting_reference as ref
import robust_cost_reference as rc
from conftest import DATA, to_product_measurements
from test_launch_geometry_gpu import DR, Handle, device_input, guard_of, library_options
from test_parity_gpu import _grid2d_measurements, _inject_outliers, _random_graph
from test_reweighting_gpu import Edges, _bits, _expected_counts, _graph257, _iterates, _max_ratio, _q_values

pytestmark = pytest.mark.gpu

LD = np.longdouble
TYPES = rc.TYPES


def _report(case, what, ratio):
    print("ratio %-30s %-12s %.3e" % (case, what, ratio))
    return ratio


class REdges(Edges):
    """The geometry suite's edge registration plus the new entry."""

    def robust(self, Xd, cost, w_tol=1e-8, update=True, nbr=None, stats=True):
        L = self.h.L
        c = cost if isinstance(cost, L.RobustCostC) or cost is None else rc.to_c(L, cost)
        st = L.ReweightStatsC(-1, -1, -1, -1, -1.0, -1.0)
        rcode = self.h.lib.dpgo_problem_robust_reweight_device(self.h.h, L.ptr(Xd), L.ptr(nbr), None if c is None else C.byref(c),
                                                               float(w_tol), int(update), C.byref(st) if stats else None)
        return rcode, st


def _counts(st):
    return (st.inliers, st.outliers, st.undecided)


def _costs_for(rsq_free):
    """One Cost per type with thresholds from the residuals' quantiles: Huber and TLS at the median, GNC_TLS with its
    bounds at the 30 % / 70 % quantiles."""
    rsq_free = np.asarray(rsq_free, dtype=np.float64)
    c = float(np.sqrt(np.quantile(rsq_free, 0.5)))
    if len(rsq_free) >= 10:
        mu, barc = ref.tls_parameters_for(rsq_free)
    else:  # (a single edge: between the bounds)
        mu, barc = 0.7, float(np.sqrt(max(rsq_free.max(), 1e-30)))
    return [rc.Cost("L2"), rc.Cost("L1"), rc.Cost("TLS", tls=c), rc.Cost("Huber", huber=c), rc.Cost("GM"),
            rc.Cost("GNC_TLS", mu=mu, barc=barc)]


def _branch_shares(cost, rsq_free):
    r = np.sqrt(np.asarray(rsq_free, dtype=np.float64))
    if cost.type in ("Huber", "TLS"):
        below = float((r < (cost.huber if cost.type == "Huber" else cost.tls)).mean())
        return [below, 1.0 - below]
    if cost.type == "GNC_TLS":
        return list(np.bincount(ref.tls_branches(rsq_free, cost.mu, cost.barc), minlength=3) / float(len(r)))
    return [1.0]


def _check_weights(case, cost, rsq_dev, w_dev, w_before, fixed):
    """The weights of one update against the longdouble weight of the DEVICE's rsq: k EPS w, exact where the bound is zero
    (L2, TLS, the saturated branches) further than 4 ulp from a threshold; there either neighbouring branch; fixed edges
    bitwise untouched."""
    free = ~fixed
    assert np.array_equal(_bits(w_dev[fixed]), _bits(w_before[fixed])), case
    want, bound, near = rc.weights_from_rsq(cost, rsq_dev)
    err = np.abs(LD(1) * w_dev - want)
    ok = err <= bound
    for s in (-1, 1):  # within 4 ulp of a threshold: the branch of the other side is accepted too
        alt = rc.weight(cost, np.sqrt(rc._ld(rsq_dev)) * (1 + s * LD(16 * rc.EPS)))
        ok |= near & (np.abs(LD(1) * w_dev - alt) <= rc.weight_bound(cost, alt) + 16 * rc.EPS * np.abs(alt))
    sel = free & ~near
    _report(case, "weight", _max_ratio(err[sel], bound[sel]))
    assert ok[free].all(), (case, cost)
    sat = sel & ((want == 0) | (want == 1))
    assert np.array_equal(_bits(w_dev[sat]), _bits(np.asarray(want[sat], dtype=np.float64))), case


def _check_cost(case, what, got, cost, rsq_ref, rsq_bound, weights, fixed, counted, grid=None):
    want, bound = rc.cost_reference(cost, rsq_ref, rsq_bound, weights, fixed, counted, grid)
    ratio = _report(case, what, float(abs(LD(got) - want) / bound) if bound > 0 else float(got != want))
    assert ratio <= 1.0, (case, what, got, float(want), float(bound))


def _drive(case, ed, meas, fixed, iterates, d, r, w0=None, types=TYPES, grid=None):
    """Every cost type at every iterate: update = 0, update = 1, the counts at w_tol = 0.25.  Returns {(iterate, type):
    (weights, stats of the update)}."""
    guard = guard_of(d, r)
    free = ~fixed
    counted_all = np.ones(len(fixed), dtype=bool)  # private edges only: every one contributes
    out, nbr = {}, None
    for name, X in iterates:
        Xd = device_input(X, guard)
        rsq_ref, mag = ref.residuals(meas, X)
        rsq_bound = ref.rsq_bound(mag, d, r)
        rsq_ref64 = np.asarray(rsq_ref, dtype=np.float64)
        # what the GNC entry leaves on the same handle
        rcode, _, mx10 = ed.reweight(Xd, 1.0, 1.0, update=False, nbr=nbr)
        assert rcode == 0
        _, rsq10 = ed.get()
        ratio = _report("%s %s" % (case, name), "rsq", _max_ratio(np.abs(rc._ld(rsq10) - rsq_ref), rsq_bound))
        assert ratio <= 1.0
        for cost in [c for c in _costs_for(rsq_ref64[free]) if c.type in types]:
            tag = "%s %s %s" % (case, name, cost.type)
            if free.sum() >= 10:
                share = _branch_shares(cost, rsq_ref64[free])
                assert min(share) >= 0.1, (tag, share)
            wb = np.ones(len(fixed)) if w0 is None else w0
            assert ed.set(wb) == 0
            rcode, st0 = ed.robust(Xd, cost, update=False, nbr=nbr)
            assert rcode == 0, tag
            w_same, rsq_dev = ed.get()
            assert np.array_equal(_bits(w_same), _bits(wb)), tag  # update = 0: no weight changes
            assert np.array_equal(_bits(rsq_dev), _bits(rsq10)), tag  # the residual is bitwise the GNC entry's
            assert _bits([st0.max_rsq])[0] == _bits([rsq_dev.max() if len(rsq_dev) else 0.0])[0] == _bits([mx10])[0], tag
            assert _counts(st0) == _expected_counts(wb, free & counted_all, 1e-8) and st0.skipped == 0, tag
            _check_cost(tag, "cost", st0.cost, cost, rsq_ref, rsq_bound, wb, fixed, counted_all, grid)
            rcode, st1 = ed.robust(Xd, cost, update=True, nbr=nbr)
            assert rcode == 0, tag
            w_dev, rsq2 = ed.get()
            assert np.array_equal(_bits(rsq2), _bits(rsq10)) and _bits([st1.max_rsq])[0] == _bits([st0.max_rsq])[0], tag
            _check_weights(tag, cost, rsq_dev, w_dev, wb, fixed)
            assert _counts(st1) == _expected_counts(w_dev, free & counted_all, 1e-8) and st1.skipped == 0, (tag, _counts(st1))
            # rho does not depend on the weights and the fixed weights did not move: the same terms in the same tree
            assert _bits([st1.cost])[0] == _bits([st0.cost])[0], tag
            rcode, st2 = ed.robust(Xd, cost, w_tol=0.25, update=False, nbr=nbr)
            assert rcode == 0 and _counts(st2) == _expected_counts(w_dev, free & counted_all, 0.25), tag
            assert np.array_equal(_bits(ed.get()[0]), _bits(w_dev)), tag
            out[(name, cost.type)] = (w_dev, st1, cost)
    return out


# ---------------------------------------------------------------- 1. every (d, r) x every cost type
@pytest.mark.parametrize("d,r", DR)
def test_every_cost_type_matches_longdouble(oracle, d, r):
    """k_edge_robust<d, r> on 257 poses / 424 edges (two workgroups, the second ragged; hub pose; odometry fixed, with
    weights that are not 1) near the truth and at a random iterate, all six cost types with thresholds at quantiles of the
    residuals: rsq bitwise the GNC entry's, max_rsq bitwise its maximum, weights from the device's own rsq within k EPS w,
    saturated values exact, fixed weights kept bitwise, counts at w_tol 1e-8 and 0.25, the cost within its bound of the
    longdouble sum, nothing but rsq changed by update = 0."""
    om, T, hub, Qb = _graph257(oracle, d)
    rng = np.random.default_rng(300 + 10 * d + r)
    fixed = om.fixed.copy()
    w0 = np.where(fixed, rng.uniform(0.5, 1.5, om.m), rng.uniform(0.0, 1.0, om.m))
    w0[np.nonzero(~fixed)[0][:40]] = np.repeat([0.0, 1.0], 20)
    with library_options({}) as lib:
        h = Handle(lib, Qb, r, d)
        try:
            ed = REdges(h, om, np.ones(om.m), fixed)
            assert om.m == 424 and fixed.any() and (~fixed).sum() >= 100
            _drive("d%d r%d n257" % (d, r), ed, om, fixed, _iterates(oracle, T, d, r, 7 + r), d, r, w0=w0)
        finally:
            h.close()


# ---------------------------------------------------------------- 2. GNC_TLS: the new entry against the old one
@pytest.mark.parametrize("d,r", DR)
def test_gnc_tls_through_the_new_entry_is_bitwise_the_old_one(oracle, d, r):
    om, T, hub, Qb = _graph257(oracle, d)
    X = _iterates(oracle, T, d, r, 11)[1][1]
    free = ~om.fixed
    mu, barc = ref.tls_parameters_for(np.asarray(ref.residuals(om, X)[0], dtype=np.float64)[free])
    with library_options({}) as lib:
        ha, hb = Handle(lib, Qb, r, d), Handle(lib, Qb, r, d)
        try:
            Xd = device_input(X, guard_of(d, r))
            ea, eb = REdges(ha, om, np.ones(om.m), om.fixed), REdges(hb, om, np.ones(om.m), om.fixed)
            rcode, counts, mx = ea.reweight(Xd, mu, barc, update=True)
            assert rcode == 0
            rcode, st = eb.robust(Xd, rc.Cost("GNC_TLS", mu=mu, barc=barc), update=True)
            assert rcode == 0
            (wa, ra), (wb, rb) = ea.get(), eb.get()
            assert np.array_equal(_bits(wa), _bits(wb)) and np.array_equal(_bits(ra), _bits(rb))
            assert counts == _counts(st) and st.skipped == 0 and _bits([mx])[0] == _bits([st.max_rsq])[0]
            assert min(counts) >= 0.1 * free.sum()
            assert np.array_equal(_bits(_q_values(ha, Qb.nnzb)), _bits(_q_values(hb, Qb.nnzb)))
        finally:
            ha.close()
            hb.close()


# ---------------------------------------------------------------- 3. shared edges
def _three_agents(oracle, name):
    """The three-robot split of test_reweighting_gpu._agent_problem, every agent with coupling and all edges registered."""
    import dpgo_amd
    if name == "smallGrid3D":
        dataset, n = dpgo_amd.read_g2o_file(os.path.join(DATA, "smallGrid3D.g2o"))
        r = 5
    else:
        om, _, _ = _random_graph(oracle, 2, 90, 60, 20, seed=4300)
        dataset, n, r = to_product_measurements(om), 90, 3
    d = dataset.d
    ranges, per = dpgo_amd.partition_contiguous(dataset, n, 3)
    agents = []
    for a in range(3):
        pg = dpgo_amd.PoseGraph(a, r, d)
        pg.setMeasurements(per[a])
        prob = dpgo_amd.QuadraticProblem(pg, host_linear_term=False)
        slots = prob.setCouplingFromPoseGraph()
        assert prob.setReweightableEdges(include_shared=True) == len(pg.measurements())
        meas = pg.measurements()
        role, slot, slots_ref = ref.roles_and_slots(meas, a)
        assert slots_ref == [tuple(s) for s in slots]
        fixed = np.asarray(meas.fixedWeight, dtype=bool) | pg.odometry_mask(meas)
        agents.append(dict(pg=pg, prob=prob, meas=meas, role=role, slot=slot, slots=slots, fixed=fixed))
    return agents, ranges, n, d, r


@pytest.mark.parametrize("name", ["smallGrid3D", "random2D"])
def test_shared_edges_are_weighted_alike_and_counted_once(oracle, name):
    """Roles 0 / 1 / 2 through QuadraticProblem.robustReweightDevice ((d, r) = (3, 5) and (2, 3)), every agent's neighbour
    tiles = the other agents' poses of one random global iterate: an agent counts neither cost nor counts for its incoming
    shared edges, both endpoints store bitwise the same weight, and the coupling values follow the new weights."""
    import torch
    from dpgo_amd.robust import RobustCost, RobustCostParameters
    agents, ranges, n, d, r = _three_agents(oracle, name)
    rng = np.random.default_rng(41)
    Xg = oracle.polar_project(rng.standard_normal((n, d + 1, r)), d)
    by_edge, total_counts, total_edges, uncounted, outgoing = {}, np.zeros(4, dtype=np.int64), 0, 0, 0
    for a, ag in enumerate(agents):
        meas, role, slot, fixed, prob = ag["meas"], ag["role"], ag["slot"], ag["fixed"], ag["prob"]
        X = Xg[ranges[a][0]:ranges[a][1]]
        nbr_h = np.stack([Xg[ranges[rob][0] + fr] for rob, fr in ag["slots"]])
        nbr = torch.from_numpy(np.ascontiguousarray(nbr_h)).to("cuda")
        Xd = device_input(X, guard_of(d, r))
        rsq_ref, mag = ref.residuals(meas, X, nbr=nbr_h, role=role, slot=slot)
        bound = ref.rsq_bound(mag, d, r)
        free = ~fixed
        c = float(np.sqrt(np.quantile(np.asarray(rsq_ref, dtype=np.float64)[free], 0.5)))
        # (one threshold for the whole team, so that both endpoints of an edge evaluate the same function)
        if a == 0:
            huber = c
        cost = rc.Cost("Huber", huber=huber)
        host = RobustCost(RobustCostParameters("Huber", HuberThreshold=huber))
        w0, _ = prob.getEdgeWeights()
        _, crow, ccol, cvals, _ = ag["pg"].couplingMatrix()
        st = prob.robustReweightDevice(Xd, nbr, host, 1e-8, True)
        w1, rsq_dev = prob.getEdgeWeights()
        tag = "%s agent%d" % (name, a)
        ratio = _report(tag, "rsq", _max_ratio(np.abs(rc._ld(rsq_dev) - rsq_ref), bound))
        assert ratio <= 1.0
        _check_weights(tag, cost, rsq_dev, w1, w0, fixed)
        counted = role != 2
        assert (st.inliers, st.outliers, st.undecided) == _expected_counts(w1, free & counted, 1e-8) and st.skipped == 0, tag
        uncounted += int((free & ~counted).sum())
        outgoing += int((free & (role == 1)).sum())
        _check_cost(tag, "cost", st.cost, cost, rsq_ref, bound, w1, fixed, counted)
        total_counts += [st.inliers, st.outliers, st.undecided, st.skipped]
        total_edges += int((free & counted).sum())
        for e in np.nonzero(role != 0)[0]:
            by_edge.setdefault((int(meas.r1[e]), int(meas.p1[e]), int(meas.r2[e]), int(meas.p2[e])), []).append(w1[e])
        # the coupling blocks follow the weights
        prob.updateLinearMatrixFromNeighbors(nbr)
        zero = torch.zeros((ag["pg"].n(), d + 1, r), dtype=torch.float64, device="cuda")
        out = torch.empty_like(zero)
        torch.cuda.synchronize()
        prob.spmmDevice(zero, out, add_G=True)
        torch.cuda.synchronize()
        C1, Mc, cc = ref.rebuilt_C(crow, ccol, len(ag["slots"]), cvals, meas, w0, w1, role, slot)
        Gw = ref.block_product(crow, ccol, C1, nbr_h)
        bG = ref.product_bound(crow, ccol, ref.value_bound(Mc, cc, d), nbr_h, Gw)
        ratio = _report(tag, "G(w1)", ref.fro(ref._ld(out.cpu().numpy()) - Gw) / bG)
        assert ratio <= 1.0, tag
    assert by_edge and all(len(v) == 2 and _bits([v[0]])[0] == _bits([v[1]])[0] for v in by_edge.values())
    # every free edge of the team is counted exactly once: a free shared edge at its source, not at its destination
    assert total_counts.sum() == total_edges and uncounted == outgoing > 0


# ---------------------------------------------------------------- 4. launch geometry
def test_forced_grids_give_the_same_weights_and_a_repeatable_cost(oracle):
    """DPGO_GRID_EDGES = 1, 2, 3 on the 424-edge case at (3, 5): the grid-stride loop takes a second trip at 1; weights and
    counts as on the default grid, the cost within its bound at that grid's summation depth and bitwise the same in two
    runs."""
    d, r = 3, 5
    om, T, hub, Qb = _graph257(oracle, d)
    its = _iterates(oracle, T, d, r, 5)[1:]
    base = {}
    for grid in (0, 1, 2, 3):
        with library_options({"DPGO_GRID_EDGES": str(grid)} if grid else {}) as lib:
            h = Handle(lib, Qb, r, d)
            try:
                ed = REdges(h, om, np.ones(om.m), om.fixed)
                got = _drive("grid %d" % grid, ed, om, om.fixed.copy(), its, d, r, types=("Huber", "GM"),
                             grid=min(grid, 2) if grid else None)
                Xd = device_input(its[0][1], guard_of(d, r))
                for key, (w, st, cost) in got.items():
                    again = [ed.robust(Xd, cost, update=False)[1].cost for _ in range(2)]
                    assert _bits([again[0]])[0] == _bits([again[1]])[0] == _bits([st.cost])[0], (grid, key)
                    if not grid:
                        base[key] = (w, _counts(st))
                    else:
                        assert np.array_equal(_bits(w), _bits(base[key][0])) and _counts(st) == base[key][1], (grid, key)
            finally:
                h.close()


def test_grid_96x96_fills_more_than_one_wave_of_the_finish_kernel(oracle):
    """18 240 edges at (2, 3): 72 workgroups, so the finish kernel sums 72 records over two of its waves."""
    d, r = 2, 3
    om, n = _grid2d_measurements(oracle, 96, 96, seed=12)
    assert om.m == 18240 and rc.default_grid(om.m) == 72
    om.fixed = om.p1 + 1 == om.p2
    Qb = oracle.construct_Q(n, d, om)
    X = oracle.polar_project(np.random.default_rng(3).standard_normal((n, d + 1, r)), d)
    with library_options({}) as lib:
        h = Handle(lib, Qb, r, d)
        try:
            ed = REdges(h, om, np.ones(om.m), om.fixed)
            _drive("grid96", ed, om, om.fixed.copy(), [("random", X)], d, r, types=("L1", "Huber", "GM"))
        finally:
            h.close()


@pytest.mark.parametrize("d,r", [(2, 3), (3, 5)])
def test_one_edge_and_no_edge(oracle, d, r):
    om2, T2, _ = _random_graph(oracle, d, 2, 0, 0, seed=4200 + d)
    with library_options({}) as lib:
        h = Handle(lib, oracle.construct_Q(2, d, om2), r, d)
        try:
            fixed1 = np.zeros(1, dtype=bool)
            ed = REdges(h, om2, np.ones(1), fixed1)
            _drive("d%d r%d m1" % (d, r), ed, om2, fixed1, _iterates(oracle, T2, d, r, 3), d, r)
            empty = REdges(h, om2.subset([]), np.zeros(0), np.zeros(0, dtype=bool))
            Xd = device_input(_iterates(oracle, T2, d, r, 3)[0][1], guard_of(d, r))
            for update in (True, False):
                rcode, st = empty.robust(Xd, rc.Cost("Huber"), update=update)
                assert (rcode, st.inliers, st.outliers, st.undecided, st.skipped, st.max_rsq, st.cost) == (0, 0, 0, 0, 0, 0.0, 0.0)
        finally:
            h.close()


# ---------------------------------------------------------------- 5. degenerate L1 and exact values
@pytest.mark.parametrize("d,r", [(2, 2), (3, 5)])
def test_l1_at_a_zero_residual_is_skipped_and_exact_integer_cases(oracle, d, r):
    """Identity rotations, t = 0, unit precisions.  p_j = p_i: rSq == 0.0, the L1 weight would be inf -- it is not stored,
    the edge is counted as skipped and Q stays finite.  p_j - p_i = (3, 0, ..): rsq == 9.0, L1 1/3 within 2 EPS, Huber(3)
    exactly 1 (r < c is false, c / r = 1.0), TLS(3) exactly 0, GM exactly 1/100."""
    om2, _, _ = _random_graph(oracle, d, 2, 0, 0, seed=4200 + d)
    Qb = oracle.construct_Q(2, d, om2)
    z = np.zeros(1, dtype=np.int64)
    fixed1 = np.zeros(1, dtype=bool)
    exact = oracle.Measurements(d, z, z.copy(), z.copy(), z + 1, np.eye(d)[None], np.zeros((1, d)), np.ones(1), np.ones(1),
                                np.ones(1), fixed1)
    with library_options({}) as lib:
        h = Handle(lib, Qb, r, d)
        try:
            ed = REdges(h, exact, np.ones(1), fixed1)
            X = np.zeros((2, d + 1, r))
            X[:, :d, :d] = np.eye(d)
            X[:, d, 1] = 0.5
            Xd = device_input(X, guard_of(d, r))
            assert ed.set(np.array([0.75])) == 0
            rcode, st = ed.robust(Xd, rc.Cost("L1"), update=True)
            w, rsq = ed.get()
            assert rcode == 0 and rsq[0] == 0.0 and st.skipped == 1 and _counts(st) == (0, 0, 0) and w[0] == 0.75
            assert st.cost == 0.0 and st.max_rsq == 0.0
            assert np.isfinite(_q_values(h, Qb.nnzb)).all()
            X[1, d, 0] = 3.0
            Xd = device_input(X, guard_of(d, r))
            for cost, want in [(rc.Cost("L1"), None), (rc.Cost("Huber", huber=3.0), 1.0), (rc.Cost("TLS", tls=3.0), 0.0),
                               (rc.Cost("GM"), 1.0 / 100.0), (rc.Cost("L2"), 1.0)]:
                assert ed.set(np.array([0.75])) == 0
                rcode, st = ed.robust(Xd, cost, update=True)
                w, rsq = ed.get()
                assert rcode == 0 and rsq[0] == 9.0 and st.max_rsq == 9.0 and st.skipped == 0, cost
                if want is None:
                    assert abs(w[0] - 1.0 / 3.0) <= 2 * rc.EPS / 3.0, w
                else:
                    assert _bits(w)[0] == _bits([want])[0], (cost, w)
                assert _counts(st) == _expected_counts(w, ~fixed1, 1e-8)
                assert st.cost == float(rc.rho(cost, LD(3))), (cost, st.cost)  # 4.5, 3, 4.5, 4.5, 0.45: exact or one rounding
                assert np.isfinite(_q_values(h, Qb.nnzb)).all()
        finally:
            h.close()


# ---------------------------------------------------------------- 6. argument checks
def test_bad_arguments_are_refused_before_any_launch(oracle):
    import dpgo_amd.lib as L
    d, r = 3, 5
    om, T, hub, Qb = _graph257(oracle, d)
    X = _iterates(oracle, T, d, r, 1)[1][1]
    nan = float("nan")
    with library_options({}) as lib:
        h = Handle(lib, Qb, r, d)
        try:
            Xd = device_input(X, guard_of(d, r))
            none = REdges.__new__(REdges)
            none.h, none.m = h, 0
            assert none.robust(Xd, rc.Cost("Huber"))[0] == L.ERR_STATE  # no edges registered
            ed = REdges(h, om, np.ones(om.m), om.fixed)
            assert ed.robust(Xd, rc.Cost("Huber"), update=True)[0] == 0
            w_now, rsq_now = ed.get()
            Xo = device_input(_iterates(oracle, T, d, r, 2)[1][1], guard_of(d, r))
            bad = [L.RobustCostC(6, 1.0, 1.0, 1.0, 1.0), L.RobustCostC(-1, 1.0, 1.0, 1.0, 1.0)]
            bad += [rc.Cost("Huber", huber=v) for v in (0.0, -1.0, nan)] + [rc.Cost("TLS", tls=v) for v in (0.0, -1.0, nan)]
            bad += [rc.Cost("GNC_TLS", mu=v, barc=1.0) for v in (0.0, -1.0, nan)]
            bad += [rc.Cost("GNC_TLS", mu=1.0, barc=v) for v in (0.0, -1.0, nan)]
            for update in (True, False):
                for cost in bad:
                    assert ed.robust(Xo, cost, update=update)[0] == L.ERR_INVALID, cost
                assert ed.robust(None, rc.Cost("Huber"), update=update)[0] == L.ERR_INVALID
                assert ed.robust(Xo, None, update=update)[0] == L.ERR_INVALID
                assert ed.robust(Xo, rc.Cost("Huber"), update=update, stats=False)[0] == L.ERR_INVALID
                assert ed.robust(Xo, rc.Cost("Huber"), w_tol=nan, update=update)[0] == L.ERR_INVALID
            st = L.ReweightStatsC()
            c = rc.to_c(L, rc.Cost("Huber"))
            assert lib.dpgo_problem_robust_reweight_device(None, L.ptr(Xo), None, C.byref(c), 1e-8, 1, C.byref(st)) == L.ERR_INVALID
            assert lib.dpgo_problem_robust_reweight(h.h, None, C.byref(c), 1e-8, 1, C.byref(st)) == L.ERR_INVALID
            w_after, rsq_after = ed.get()
            assert np.array_equal(_bits(w_after), _bits(w_now)) and np.array_equal(_bits(rsq_after), _bits(rsq_now))
            # the host flavour on private edges says what the device flavour says
            assert lib.dpgo_problem_robust_reweight(h.h, L.ptr(np.ascontiguousarray(X)), C.byref(c), 1e-8, 0, C.byref(st)) == 0
            assert np.array_equal(_bits(ed.get()[1]), _bits(rsq_now)) and np.array_equal(_bits(ed.get()[0]), _bits(w_now))
        finally:
            h.close()


def test_shared_edges_need_the_neighbour_tiles(oracle):
    import dpgo_amd.lib as L
    from test_reweighting_gpu import _agent_problem
    pg, prob, meas, role, slot, slots, fixed, d, r = _agent_problem(oracle, "random2D", 1)
    X = oracle.polar_project(np.random.default_rng(5).standard_normal((pg.n(), d + 1, r)), d)
    Xd = device_input(X, guard_of(d, r))
    w_now, _ = prob.getEdgeWeights()
    st, c = L.ReweightStatsC(), rc.to_c(L, rc.Cost("GM"))
    assert prob._lib.dpgo_problem_robust_reweight_device(prob.handle, L.ptr(Xd), None, C.byref(c), 1e-8, 1, C.byref(st)) == L.ERR_INVALID
    assert prob._lib.dpgo_problem_robust_reweight(prob.handle, L.ptr(np.ascontiguousarray(X)), C.byref(c), 1e-8, 1,
                                                  C.byref(st)) == L.ERR_STATE
    assert np.array_equal(_bits(prob.getEdgeWeights()[0]), _bits(w_now))


# ---------------------------------------------------------------- 7. majorise-minimise, single agent
_MM = {}


def _mm_case(oracle):
    """synthetic_grid(6, 6, 6) + 20 outlier loop closures, odometry fixed; chordal start of the clean graph at r = 5."""
    if not _MM:
        om, n, _ = oracle.synthetic_grid(6, 6, 6, seed=0)
        allm = _inject_outliers(oracle, om, n, 20, seed=5)
        allm.fixed = allm.p1 + 1 == allm.p2
        _MM.update(allm=allm, n=n, X0=np.ascontiguousarray(oracle.lift(oracle.chordal_initialization(om, n), 5)))
    return _MM["allm"], _MM["n"], _MM["X0"]


@pytest.mark.parametrize("ctype", ["L1", "Huber", "TLS", "GM"])
def test_irls_rounds_never_raise_the_robust_cost(oracle, ctype):
    """Eight rounds of (solve from the current iterate; robustReweightDevice(update=True)) at the reference's default
    thresholds.  Every rho here is concave in r^2, so the weighted cost at the new weights majorises it and touches it at
    the iterate the weights came from; RTR accepts only decreases of the weighted cost: cost_{k+1} <= cost_k + slack, slack
    = 1e-9 cost_0 for the rounding of RTR's own decrease test (differences of f of order EPS |Q| |X|^2, many orders
    below)."""
    import torch
    import dpgo_amd
    from dpgo_amd.robust import RobustCost, RobustCostParameters
    allm, n, X0 = _mm_case(oracle)
    r, d = 5, allm.d
    pg = dpgo_amd.PoseGraph(0, r, d)
    pg.setMeasurements(to_product_measurements(allm))
    assert pg.n() == n
    prob = dpgo_amd.QuadraticProblem(pg)
    assert prob.setReweightableEdges() == allm.m
    opt = dpgo_amd.QuadraticOptimizer(prob, dpgo_amd.ROptParameters())
    cost = RobustCost(RobustCostParameters(ctype))
    free = ~np.asarray(pg.measurements().fixedWeight, dtype=bool)
    assert free.sum() == (~allm.fixed).sum() > 20
    Xd = torch.from_numpy(X0.copy()).to("cuda")
    torch.cuda.synchronize()
    costs = []
    for k in range(8):
        opt.optimizeDevice(Xd)
        st = prob.robustReweightDevice(Xd, None, cost, 1e-8, True)
        costs.append(st.cost)
        w, rsq = prob.getEdgeWeights()
        assert st.skipped == 0 and st.inliers + st.outliers + st.undecided == free.sum()
        if k == 0:
            assert (w[free] != 1.0).any() and (w[~free] == 1.0).all()
        f, _ = prob.evalDevice(Xd)
        half = 0.5 * float(np.sum(w * rsq))
        assert abs(f - half) <= 1e-10 * half, (ctype, k, f, half)
    slack = 1e-9 * costs[0]
    worst = max((costs[k + 1] - costs[k]) / slack for k in range(7))
    print("ratio %-30s %-12s %.3e" % ("irls " + ctype, "rise/slack", worst))
    print("costs", ctype, costs)
    assert worst <= 1.0, (ctype, costs)
    assert costs[-1] < costs[0]


# ---------------------------------------------------------------- 8. two agents on one GPU
@pytest.mark.parametrize("ctype", ["Huber", "GM"])
def test_two_agents_follow_the_protocol_and_never_raise_the_global_cost(oracle, ctype):
    """The same graph cut in two, DistributedRobustPGO with four weight updates of at most six inner iterations: exactly
    four updates, the global robust cost of info non-increasing (slack as above; both blocks' solves decrease the same
    global weighted cost, one colour at a time) and equal to the longdouble cost of the gathered iterates within the
    bound."""
    import dpgo_amd
    from dpgo_amd.agent import DeviceAgent, ExchangePlan, PGOAgentParameters, RBCDCluster, build_pose_graphs
    from dpgo_amd.robust import DistributedRobustPGO, RobustCostParameters
    allm, n, X0 = _mm_case(oracle)
    r, d, robots = 5, allm.d, 2
    pm = to_product_measurements(allm)
    pm.fixedWeight[:] = False  # (the agent path fixes odometry by itself)
    ranges, graphs = build_pose_graphs(pm, n, robots, r)
    plan = ExchangePlan(graphs)
    agents = {a: DeviceAgent(graphs, plan, a, X0[ranges[a][0]:ranges[a][1]], dpgo_amd.ROptParameters(precond="jacobi"))
              for a in range(robots)}
    drv = DistributedRobustPGO(RBCDCluster(plan, agents), RobustCostParameters(ctype),
                               PGOAgentParameters(robustOptNumWeightUpdates=4, robustOptInnerIters=6, maxNumIters=40))
    iterates = []
    info = drv.run(on_update=lambda rec: iterates.append(
        np.concatenate([agents[a].iterate_in_caller_order().cpu().numpy() for a in range(robots)], axis=0)))
    assert info["updates"] == 4 and len(info["history"]) == 4 and len(iterates) == 4
    assert all(1 <= k <= 6 for k in info["inner_iterations"]) and info["iterations"] <= 40
    costs = [h["cost"] for h in info["history"]]
    slack = 1e-9 * costs[0]
    worst = max((costs[k + 1] - costs[k]) / slack for k in range(3))
    print("ratio %-30s %-12s %.3e" % ("two agents " + ctype, "rise/slack", worst))
    assert worst <= 1.0, costs
    assert info["robust_cost"] <= costs[-1] + slack
    robot = np.searchsorted([rg[1] for rg in ranges], np.arange(n), side="right")
    fixed = (robot[allm.p1] == robot[allm.p2]) & (allm.p1 + 1 == allm.p2)
    cost = rc.Cost(ctype)
    for k, X in enumerate(iterates):
        rsq_ref, mag = ref.residuals(allm, X)
        h = info["history"][k]
        _check_cost("two agents %s update %d" % (ctype, k), "cost", h["cost"], cost, rsq_ref, ref.rsq_bound(mag, d, r),
                    np.ones(allm.m), fixed, np.ones(allm.m, dtype=bool), grid=1)
        assert h["inliers"] + h["outliers"] + h["undecided"] == (~fixed).sum() and h["skipped"] == 0


# ---------------------------------------------------------------- 9. memory
def test_record_buffers_are_released_with_the_handle(oracle):
    import dpgo_amd.lib as L
    d, r = 3, 5
    om, T, hub, Qb = _graph257(oracle, d)
    X = _iterates(oracle, T, d, r, 1)[1][1]

    def live(lib):
        a, b = C.c_longlong(-1), C.c_longlong(-1)
        assert lib.dpgo_debug_live_allocations(C.byref(a), C.byref(b)) == L.OK
        return a.value, b.value

    with library_options({}) as lib:
        start = live(lib)
        h = Handle(lib, Qb, r, d)
        ed = REdges(h, om, np.ones(om.m), om.fixed)
        registered = live(lib)
        assert ed.robust(device_input(X, guard_of(d, r)), rc.Cost("GM"), update=True)[0] == 0
        used = live(lib)
        assert used[0] >= registered[0] + 2 and used[1] >= registered[1] + 32 * 1024 + 32  # the records and the result
        ed2 = REdges(h, om, np.ones(om.m), om.fixed)  # a new registration drops them with the old one
        assert live(lib)[0] <= used[0] - 2 and ed2.m == om.m
        h.close()
        assert live(lib) == start
