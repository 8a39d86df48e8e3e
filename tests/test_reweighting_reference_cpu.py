"""The longdouble restatement of the GNC re-weighting path (reweighting_reference.py) against the oracle's fp64 code on small
random graphs, 2-D and 3-D, single agent and one agent's block of a three-robot split; and its a-priori bounds against a
second fp64 implementation that sums in another order (no GPU needed)."""
import numpy as np
import pytest

import reweighting_reference as ref
from test_parity_gpu import _random_graph

N, N_LC, HUB = 40, 20, 10


def _graph(oracle, d):
    om, T, hub = _random_graph(oracle, d, N, N_LC, HUB, seed=900 + d)
    return om, T


def _weights(rng, m, fixed):
    """One third of the free edges at 0, one third in [0.05, 1], the rest at 1; fixed edges keep 1."""
    w = np.ones(m)
    free = np.nonzero(~np.asarray(fixed, dtype=bool))[0]
    k = len(free) // 3
    pick = rng.permutation(free)
    w[pick[:k]] = 0.0
    w[pick[k:2 * k]] = rng.uniform(0.05, 1.0, k)
    return w


def _with_weights(om, w):
    out = om.subset(np.arange(om.m))
    out.weight = np.asarray(w, dtype=np.float64).copy()
    return out


def _agent_block(oracle, d, a, robots=3):
    """(edges of agent a in local indices, role, slot, slots, block size, global range) of the split graph."""
    om, T = _graph(oracle, d)
    ranges, per = oracle.partition_contiguous(om, N, robots)
    meas = oracle.Measurements.concat([per[a]["odometry"], per[a]["private"], per[a]["shared"]])
    role, slot, slots = ref.roles_and_slots(meas, a)
    assert (role != 0).any() and (a != 1 or ((role == 1).any() and (role == 2).any()))  # (the hub lives in block 1)
    return meas, role, slot, slots, ranges[a][1] - ranges[a][0], ranges, per[a]


@pytest.mark.parametrize("d,r", [(2, 2), (2, 3), (3, 3), (3, 5)])
def test_residuals_match_the_oracle(oracle, d, r):
    """rSq of every edge at the noisy ground truth (cancellation) and at a random point: the oracle's fp64
    measurement_error is within the a-priori bound c_rsq u mag of the longdouble restatement."""
    om, T = _graph(oracle, d)
    rng = np.random.default_rng(5 + r)
    for X in (oracle.polar_project(oracle.lift(T, r) + 1e-3 * rng.standard_normal((N, d + 1, r)), d),
              oracle.polar_project(rng.standard_normal((N, d + 1, r)), d)):
        rsq, mag = ref.residuals(om, X)
        err = np.abs(ref._ld(oracle.measurement_error(om, X)) - rsq)
        assert (err <= ref.rsq_bound(mag, d, r)).all(), float((err / ref.rsq_bound(mag, d, r)).max())
        assert (rsq >= 0).all() and (mag >= rsq).all()


@pytest.mark.parametrize("d", [2, 3])
def test_shared_edge_residuals_take_the_neighbours_pose(oracle, d):
    """Roles 1 and 2: with the neighbour tiles filled from the global iterate, an agent's residuals are the central
    graph's residuals of the same edges."""
    r = d + 1
    om, T = _graph(oracle, d)
    X = oracle.polar_project(np.random.default_rng(3).standard_normal((N, d + 1, r)), d)
    for a in range(3):
        meas, role, slot, slots, na, ranges, _ = _agent_block(oracle, d, a)
        s = ranges[a][0]
        nbr = np.stack([X[ranges[q][0] + f] for q, f in slots])
        rsq, _ = ref.residuals(meas, X[s:s + na], nbr, role, slot)
        # the same edges in global indices
        glob = meas.subset(np.arange(meas.m))
        glob.p1 = np.array([ranges[q][0] for q in meas.r1]) + meas.p1
        glob.p2 = np.array([ranges[q][0] for q in meas.r2]) + meas.p2
        want, mag = ref.residuals(glob, X)
        assert np.array_equal(rsq, want)
        assert (np.abs(ref._ld(oracle.measurement_error(glob, X)) - rsq) <= ref.rsq_bound(mag, d, r)).all()


def test_tls_weight_is_the_oracles_bit_for_bit(oracle):
    rng = np.random.default_rng(0)
    rsq = np.concatenate([rng.uniform(0, 50, 2000), 10.0 ** rng.uniform(-12, 6, 2000), [0.0, 9.0, 25.0]])
    for mu, barc in [(0.125, 1.0), (1.0, 5.0), (3.7, 2.2), (1e-4, 5.0), (1e4, 0.3)]:
        got = ref.tls_weight_fp64(rsq, mu, barc)
        want = oracle.gnc_tls_weight(np.sqrt(rsq), mu, barc)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (mu, barc)
        assert ((got >= 0) & (got <= 1)).all()
        br = ref.tls_branches(rsq, mu, barc)
        assert (got[br == 0] == 1.0).all() and (got[br == 2] == 0.0).all()
    # rSq0 = 9 = upper exactly (mu = 1/8, barc = 1): weight 0
    assert ref.tls_thresholds(0.125, 1.0)[1] == 9.0 and ref.tls_weight_fp64(np.array([9.0]), 0.125, 1.0)[0] == 0.0
    # the thresholds chosen from quantiles put the asked share of edges into each branch
    mu, barc = ref.tls_parameters_for(rsq[:2000])
    share = np.bincount(ref.tls_branches(rsq[:2000], mu, barc), minlength=3) / 2000.0
    assert (np.abs(share - [0.3, 0.4, 0.3]) < 0.01).all(), share


def _fp64_two_step(rowptr, colidx, ncols, vals0, meas, w0, w1, targets):
    """The two-step rebuild in fp64, contributions formed by numpy's own products and summed last edge first."""
    def blocks(w):
        m, d = meas.m, meas.d
        b = d + 1
        T = np.zeros((m, b, b))
        T[:, :d, :d], T[:, :d, d], T[:, d, d] = meas.R, meas.t, 1.0
        om = np.concatenate([np.repeat((w * meas.kappa)[:, None], d, 1), (w * meas.tau)[:, None]], axis=1)
        TO = T * om[:, None, :]
        Om = np.zeros((m, b, b))
        Om[:, np.arange(b), np.arange(b)] = om
        return TO @ np.swapaxes(T, 1, 2), Om, -TO, -np.swapaxes(TO, 1, 2)
    out = np.array(vals0, dtype=np.float64, copy=True)
    for w, sign in ((w0, -1.0), (w1, 1.0)):
        K = blocks(np.asarray(w, dtype=np.float64))
        acc = np.zeros_like(out)
        for e, kind, rows, cols in reversed(targets):
            if len(e):
                s = ref.find_slots(rowptr, colidx, ncols, rows, cols)
                np.add.at(acc, s[::-1], K[kind][e[::-1]])
        out = out + sign * acc
    return out


@pytest.mark.parametrize("d", [2, 3])
def test_rebuilt_Q_matches_construction_at_the_new_weights(oracle, d):
    """base + contributions(w1) on Q(w0)'s values: oracle.construct_Q at w1, and an fp64 two-step rebuild that sums in
    another order, are both within c_slot u M of the longdouble result; the hub's diagonal slot counts every hub edge."""
    om, T = _graph(oracle, d)
    rng = np.random.default_rng(d)
    w0 = np.where(om.fixed, 1.0, rng.uniform(0.2, 1.0, om.m))
    w1 = _weights(rng, om.m, om.fixed)
    w1[np.nonzero(~om.fixed)[0][-1]] = 1e-12
    Q0 = oracle.construct_Q(N, d, _with_weights(om, w0))
    Q1 = oracle.construct_Q(N, d, _with_weights(om, w1))
    assert np.array_equal(Q0.colidx, Q1.colidx)
    got, M, count = ref.rebuilt_Q(Q0.rowptr, Q0.colidx, Q0.vals, om, w0, w1)
    bound = ref.value_bound(M, count, d)
    assert count.sum() == 4 * om.m and count.max() >= HUB
    assert (np.abs(ref._ld(Q1.vals) - got) <= bound).all()
    two = _fp64_two_step(Q0.rowptr, Q0.colidx, N, Q0.vals, om, w0, w1, ref.q_targets(om))
    ratio = float((np.abs(ref._ld(two) - got)[bound > 0] / bound[bound > 0]).max())
    assert ratio <= 1.0, ratio
    assert (np.abs(ref._ld(two) - got)[bound == 0] == 0).all()
    # w1 = w0 gives the values back to within the bound as well, and M >= |values|
    same, M0, _ = ref.rebuilt_Q(Q0.rowptr, Q0.colidx, Q0.vals, om, w0, w0)
    assert (np.abs(same - ref._ld(Q0.vals)) <= ref.value_bound(M0, count, d)).all() and (M0 >= np.abs(Q0.vals)).all()


@pytest.mark.parametrize("d", [2, 3])
def test_rebuilt_agent_block_matches_construct_Q_and_construct_G(oracle, d):
    """One agent's block with shared edges of both roles: rebuilt Q against oracle.construct_Q(private, shared) and
    G = C(w1) * neighbour tiles against oracle.construct_G at the new weights, within the value and product bounds."""
    r = d + 2
    for a in range(3):
        meas, role, slot, slots, na, ranges, per = _agent_block(oracle, d, a)
        rng = np.random.default_rng(10 * d + a)
        fixed = meas.fixed | (meas.p1 + 1 == meas.p2) & (role == 0)
        w0 = np.where(fixed, 1.0, rng.uniform(0.2, 1.0, meas.m))
        w1 = _weights(rng, meas.m, fixed)
        n_own = per["odometry"].m + per["private"].m

        def split(w):
            m = _with_weights(meas, w)
            return m.subset(np.arange(n_own)), m.subset(np.arange(n_own, meas.m))
        Q0 = oracle.construct_Q(na, d, *split(w0), my_id=a)
        Q1 = oracle.construct_Q(na, d, *split(w1), my_id=a)
        got, M, count = ref.rebuilt_Q(Q0.rowptr, Q0.colidx, Q0.vals, meas, w0, w1, role)
        assert count.sum() == 4 * int((role == 0).sum()) + int((role != 0).sum())
        assert (np.abs(ref._ld(Q1.vals) - got) <= ref.value_bound(M, count, d)).all()
        two = _fp64_two_step(Q0.rowptr, Q0.colidx, na, Q0.vals, meas, w0, w1, ref.q_targets(meas, role))
        assert (np.abs(ref._ld(two) - got) <= ref.value_bound(M, count, d)).all()
        # coupling blocks: pattern from the shared edges; the values at w0 are this module's own, rounded to fp64
        sh = np.nonzero(role != 0)[0]
        mine = np.where(role[sh] == 1, meas.p1[sh], meas.p2[sh])
        key = np.unique(mine.astype(np.int64) * len(slots) + slot[sh])
        rows, cols = key // len(slots), key % len(slots)
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=na))])
        zero = np.zeros((len(key), d + 1, d + 1))
        C0 = ref.rebuilt_C(rowptr, cols, len(slots), zero, meas, 0 * w0, w0, role, slot)[0].astype(np.float64)
        C1, Mc, cc = ref.rebuilt_C(rowptr, cols, len(slots), C0, meas, w0, w1, role, slot)
        assert cc.sum() == len(sh)
        nbr = oracle.polar_project(rng.standard_normal((len(slots), d + 1, r)), d)
        G = ref.block_product(rowptr, cols, C1, nbr)
        want = oracle.construct_G(na, d, r, split(w1)[1], a, {pid: nbr[k] for k, pid in enumerate(slots)})
        assert ref.fro(ref._ld(want) - G) <= ref.product_bound(rowptr, cols, ref.value_bound(Mc, cc, d), nbr, G)
        two = _fp64_two_step(rowptr, cols, len(slots), C0, meas, w0, w1, ref.c_targets(meas, role, slot))
        assert (np.abs(ref._ld(two) - C1) <= ref.value_bound(Mc, cc, d)).all()


@pytest.mark.parametrize("d", [2, 3])
def test_product_bound_holds_for_an_fp64_product(oracle, d):
    """scipy's fp64 product with the fp64 two-step values stays inside the product bound of the longdouble Q(w1) V."""
    r = d + 1
    om, T = _graph(oracle, d)
    rng = np.random.default_rng(7)
    w0, w1 = np.ones(om.m), _weights(rng, om.m, om.fixed)
    Q0 = oracle.construct_Q(N, d, om)
    got, M, count = ref.rebuilt_Q(Q0.rowptr, Q0.colidx, Q0.vals, om, w0, w1)
    V = rng.standard_normal((N, d + 1, r))
    want = ref.block_product(Q0.rowptr, Q0.colidx, got, V)
    two = _fp64_two_step(Q0.rowptr, Q0.colidx, N, Q0.vals, om, w0, w1, ref.q_targets(om))
    fp64 = (oracle.BSR(N, d + 1, Q0.rowptr, Q0.colidx, two).to_scipy().tocsr() @ V.reshape(-1, r)).reshape(V.shape)
    bound = ref.product_bound(Q0.rowptr, Q0.colidx, ref.value_bound(M, count, d), V, want)
    assert ref.fro(ref._ld(fp64) - want) <= bound
    # and the longdouble product is the oracle's at the new weights to the suite's tolerance
    Q1 = oracle.construct_Q(N, d, _with_weights(om, w1))
    assert ref.fro(ref._ld(Q1.to_scipy().tocsr() @ V.reshape(-1, r)).reshape(V.shape) - want) <= bound


@pytest.mark.parametrize("dim,precond", [(3, "jacobi"), (3, "amg"), (2, "amg")])
def test_solve_comparison_of_the_gpu_suite_is_well_posed(oracle, dim, precond):
    """tests/test_reweighting_gpu.py compares a handle whose Q was rebuilt on the device with one built from the host's
    values: the two differ in the last bits, so the solve they run must not amplify a one-ulp perturbation of Q(w1) to
    anywhere near the tolerances (iterate 1e-7, cost 1e-10).  The oracle at that suite's workload, w1 and solve
    parameters, four random perturbations: same tCG / RTR counts, iterate and cost within a hundredth of the
    tolerances.  (With block-Jacobi at the default 50 tCG steps per outer iteration the oracle itself moves by 1.5e-8 /
    1.4e-9, at three outer iterations by 2.9e-7 / 3.5e-9: a comparison at those parameters would test the trust region's
    conditioning, not the copies.)"""
    import test_reweighting_gpu as gpu
    om, n, r, X0 = gpu._workload(oracle, dim)
    d = om.d
    Q1 = oracle.construct_Q(n, d, _with_weights(om, gpu._set_w1(om)))
    kw = dict(amg_k=oracle.amg_default_ks(n, d + 1)) if precond == "amg" else {}

    def solve(Q):
        op = oracle.QuadraticProblem(Q, None, r, d, precond=precond, **kw)
        oo = oracle.QuadraticOptimizer(op, oracle.ROptParameters(RTR_iterations=gpu.RTR_ITERATIONS,
                                                                 RTR_tCG_iterations=gpu.RTR_TCG_ITERATIONS),
                                       hess_recurrence=True)
        X = oo.optimize(X0)
        return X, oo.result
    X, res = solve(Q1)
    assert res.outer_iters == gpu.RTR_ITERATIONS and res.tcg_iters > gpu.RTR_ITERATIONS
    for seed in range(4):
        eps = ref.U * np.random.default_rng(100 + seed).uniform(-1, 1, Q1.vals.shape)
        Xp, rp = solve(oracle.BSR(n, d + 1, Q1.rowptr, Q1.colidx, Q1.vals * (1 + eps)))
        assert (rp.tcg_iters, rp.outer_iters) == (res.tcg_iters, res.outer_iters)
        assert np.linalg.norm(Xp - X) <= 1e-9 * np.linalg.norm(X)
        assert abs(rp.fOpt - res.fOpt) <= 1e-12 * abs(res.fOpt)
