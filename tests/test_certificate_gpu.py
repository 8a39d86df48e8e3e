"""Certificate of global optimality on the device (dpgo_problem_certify*, QuadraticProblem.certify, solveCertifiedPGO)
against the numpy restatement of C(X) = Q - Lambda(X) (tests/certificate_reference.py) and the analytic ring."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import DATA, to_product_measurements

import certificate_reference as ref

pytestmark = pytest.mark.gpu

LAM_RING = -2 * (1 - np.cos(2 * np.pi / 16))


def _problem(om, n, r):
    import dpgo_amd
    pg = dpgo_amd.PoseGraph(0, r, om.d)
    pg.setMeasurements(to_product_measurements(om))
    assert pg.n() == n
    return dpgo_amd.QuadraticProblem(pg)


def _dataset(oracle, name):
    if name.startswith("grid:"):
        nx, ny, nz = [int(v) for v in name[5:].split("x")]
        om, n, _ = oracle.synthetic_grid(nx, ny, nz, seed=0)
        return om, n
    if name.startswith("grid2d:"):
        from test_parity_gpu import _grid2d_measurements
        return _grid2d_measurements(oracle, *[int(v) for v in name[7:].split("x")], seed=4)
    return oracle.read_g2o(os.path.join(DATA, name + ".g2o"))


@pytest.mark.parametrize("name,variant", [("smallGrid3D", "auto"), ("sphere2500", "auto"), ("grid2d:40x30", "auto"),
                                          ("grid:40x40x25", "plain"), ("grid:40x40x25", "symmetric")])
def test_certificate_apply_matches_restatement(oracle, name, variant):
    om, n = _dataset(oracle, name)
    d, r = om.d, 5
    prob = _problem(om, n, r)
    if variant != "auto":
        assert prob.setSpmmVariant(variant) == variant
    Q = ref.sparse_Q(oracle.construct_Q(n, d, om))
    rng = np.random.default_rng(7)
    X = rng.standard_normal((r, (d + 1) * n))
    V = rng.standard_normal((r, (d + 1) * n))
    got = prob.certificateApply(X, V)
    want = ref.certificate_apply(Q, X, V, d)
    assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want)


PARAMS = dict(eta=1e-6, tol_rel=1e-9, max_iterations=500, precond="jacobi", seed=3)


@pytest.mark.parametrize("d,r", [(2, 2), (2, 3), (3, 3), (3, 4), (3, 5)])
def test_twisted_ring(oracle, d, r):
    om, n = ref.ring_measurements(oracle, 16, d)
    prob = _problem(om, n, r)
    Q = ref.sparse_Q(oracle.construct_Q(n, d, om))
    X1 = ref.ring_iterate(n, d, r, winding=1)
    res = prob.certify(X1, **PARAMS)
    assert res.status == "NOT_CERTIFIED"
    assert res.lambda_min <= -PARAMS["eta"] * res.scale
    assert abs(res.lambda_min - LAM_RING) <= 1e-8
    w = res.witness.reshape(-1)
    Cm = ref.certificate_matrix(Q, X1, d).toarray()
    Z = ref.null_basis(X1, d)
    assert abs(np.linalg.norm(w) - 1) <= 1e-10
    assert np.linalg.norm(Z.T @ w) <= 1e-10
    assert abs(w @ Cm @ w - res.lambda_min) <= 1e-10
    assert res.deflated == d + 1
    X0 = ref.ring_iterate(n, d, r, winding=0)
    res0 = prob.certify(X0, **PARAMS)
    assert res0.status == "CERTIFIED" and res0.deflated == d + 1
    assert abs(res0.lambda_min + LAM_RING) <= 1e-8


_SOLVED = {}


def _solved(oracle, name, r=5):
    """(problem, X, Q, om, n) with X solved by the existing optimizer to a tight gradient norm (cached per module)."""
    if name not in _SOLVED:
        import dpgo_amd
        from conftest import tiles_to_matrix
        om, n = _dataset(oracle, name)
        prob = _problem(om, n, r)
        X = tiles_to_matrix(oracle.lift(oracle.chordal_initialization(om, n), r))
        opt = dpgo_amd.QuadraticOptimizer(prob, dpgo_amd.ROptParameters(precond="multilevel", gradnorm_tol=1e-7,
                                                                         RTR_iterations=100, RTR_tCG_iterations=500,
                                                                         time_bound_s=120.0))
        for _ in range(10):
            X = opt.optimize(X)
            if opt.getOptResult().gradNormOpt <= 1e-7:
                break
        _SOLVED[name] = (prob, X, ref.sparse_Q(oracle.construct_Q(n, om.d, om)), om, n)
    return _SOLVED[name]


@pytest.mark.parametrize("name,ref2f", [("smallGrid3D", 1025.3980556263), ("sphere2500", 1687.0058142808),
                                        ("torus3D", 24227.0455583823)])
def test_solved_datasets_certify(oracle, name, ref2f):
    import dpgo_amd
    prob, X, Q, om, n = _solved(oracle, name)
    d, r = om.d, X.shape[0]
    res = prob.certify(X, eta=1e-6, tol_rel=1e-7, max_iterations=2000, precond="multilevel")
    assert res.status == "CERTIFIED", res
    Cs = ref.certificate_matrix(Q, X, d)
    Z = ref.null_basis(X, d, rtol=1e-6)
    if n <= 1000:
        lam = ref.complement_lambda_min(Cs.toarray(), Z)
    else:
        lam = ref.complement_lambda_min_sparse(Cs, Z, res.scale)
    assert abs(res.lambda_min - lam) <= 1e-6 * res.scale, (res.lambda_min, lam)
    T = dpgo_amd.round_trajectory(X, r, d)
    Xr = np.zeros_like(X)
    Xr[:d] = T
    f, fr = prob.f(X), prob.f(Xr)
    assert fr - f >= -1e-9 * abs(f) and fr - f <= 1e-6 * abs(f)
    assert abs(2 * fr - ref2f) <= 1e-6 * ref2f


def test_preconditioners_agree_on_sphere2500(oracle):
    prob, X, _, _, _ = _solved(oracle, "sphere2500")
    out = {pc: prob.certify(X, eta=1e-6, tol_rel=1e-7, max_iterations=3000, precond=pc)
           for pc in ["none", "jacobi", "multilevel"]}
    for pc, res in out.items():
        print("sphere2500 %-10s %s lambda_min %.6e  %d its  %d products  %.1f ms" % (
            pc, res.status, res.lambda_min, res.iterations, res.products, res.elapsedMs))
    assert len({res.status for res in out.values()}) == 1
    lams = [res.lambda_min for res in out.values()]
    assert max(lams) - min(lams) <= 1e-6 * out["none"].scale
    assert out["multilevel"].products <= out["none"].products


def test_bitwise_reproducible(oracle):
    prob, X, _, _, _ = _solved(oracle, "smallGrid3D")
    a = prob.certify(X, eta=1e-6, tol_rel=1e-7, precond="multilevel")
    b = prob.certify(X, eta=1e-6, tol_rel=1e-7, precond="multilevel")
    assert a.lambda_min == b.lambda_min and a.residual == b.residual and a.iterations == b.iterations
    assert np.array_equal(a.witness, b.witness)
    om, n = ref.ring_measurements(oracle, 16, 3)
    p = _problem(om, n, 4)
    X1 = ref.ring_iterate(n, 3, 4, 1)
    a, b = p.certify(X1, **PARAMS), p.certify(X1, **PARAMS)
    assert a.lambda_min == b.lambda_min and np.array_equal(a.witness, b.witness)


@pytest.mark.parametrize("d", [2, 3])
def test_staircase_escapes_the_twisted_ring(oracle, d):
    import dpgo_amd
    om, n = ref.ring_measurements(oracle, 16, d)
    X1 = ref.ring_iterate(n, d, d, winding=1)
    out = dpgo_amd.solveCertifiedPGO(to_product_measurements(om), X0=X1, params=PARAMS)
    print("ring d=%d: %s rank %d f %.3e escapes %s" % (d, out.status, out.rank, out.f, out.escapes))
    # the first escape leaves rank d; the landscape at rank d + 1 still holds a saddle at f / 2 (the ring folded into the
    # new dimension) that the solve may settle on -- the staircase then escapes once more
    assert out.status == "CERTIFIED" and d + 1 <= out.rank <= d + 2 and len(out.escapes) == out.rank - d
    assert out.escapes[0]["rank"] == d and abs(out.escapes[0]["lambda_min"] - LAM_RING) <= 1e-8
    assert all(e["f_after"] < e["f_before"] for e in out.escapes)
    assert out.f <= 1e-10 and out.f_rounded <= 1e-10
    T = out.trajectory.reshape(d, n, d + 1)[:, :, :d]  # rotations
    for i in range(1, n):
        assert np.linalg.norm(T[:, i] - T[:, 0]) <= 1e-5


def test_staircase_smallgrid_certifies_at_r0(oracle):
    import dpgo_amd
    om, n = _dataset(oracle, "smallGrid3D")
    out = dpgo_amd.solveCertifiedPGO(to_product_measurements(om), params=dict(eta=1e-6, tol_rel=1e-7, precond="multilevel"))
    assert out.status == "CERTIFIED" and out.rank == om.d and not out.escapes
    assert abs(2 * out.f_rounded - 1025.3980556263) <= 1e-6 * 1025.3980556263


def test_staircase_rank_limit_and_unsupported_escape(oracle):
    import dpgo_amd
    import dpgo_amd.lib as L
    import torch
    om, n = ref.ring_measurements(oracle, 16, 3)
    X1 = ref.ring_iterate(n, 3, 6, winding=1)
    out = dpgo_amd.solveCertifiedPGO(to_product_measurements(om), r0=6, X0=X1, params=PARAMS)
    assert out.status == "RANK_LIMIT" and out.rank == 6 and out.certificate.status == "NOT_CERTIFIED"
    p6 = _problem(om, n, 6)
    X = torch.zeros((n * 4, 6), dtype=torch.float64, device="cuda")
    w = torch.zeros(n * 4, dtype=torch.float64, device="cuda")
    Xn = torch.zeros((n * 4, 7), dtype=torch.float64, device="cuda")
    a = C.c_double(0.0)
    rc = L.load().dpgo_certify_escape_device(p6.handle, 6, L.ptr(X), L.ptr(w), 1e-9, L.ptr(Xn), C.byref(a))
    assert rc == L.ERR_UNSUPPORTED


def test_handle_with_G_is_rejected(oracle):
    import dpgo_amd.lib as L
    om, n = ref.ring_measurements(oracle, 16, 3)
    p = _problem(om, n, 3)
    lib = L.load()
    G = np.ones((3, 4 * n), order="F")
    L.check(lib.dpgo_problem_set_G(p.handle, L.ptr(G)))
    X = np.asfortranarray(ref.ring_iterate(n, 3, 3, 1))
    cp, cr = L.CertifyParamsC(), L.CertifyResultC()
    lib.dpgo_certify_params_default(C.byref(cp))
    assert lib.dpgo_problem_certify(p.handle, L.ptr(X), C.byref(cp), C.byref(cr), None) == L.ERR_INVALID
    assert lib.dpgo_problem_certificate_apply(p.handle, L.ptr(X), L.ptr(X), L.ptr(np.empty_like(X))) == L.ERR_INVALID
    L.check(lib.dpgo_problem_set_G(p.handle, None))
    cp.tol_rel = -1.0
    assert lib.dpgo_problem_certify(p.handle, L.ptr(X), C.byref(cp), C.byref(cr), None) == L.ERR_INVALID
