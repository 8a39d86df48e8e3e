"""Certificate of global optimality: C ABI declarations, parameter defaults, host-side argument checks and the numpy
restatement of Lambda(X) / C(X) on the analytic ring (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import certificate_reference as ref


def test_header_declares_and_library_exports_certify_entries():
    import dpgo_amd.lib as L
    hdr = open(os.path.join(ROOT, "include", "dpgo_hip.h")).read()
    lib = L.load()
    for name in ["dpgo_certify_params_default", "dpgo_problem_certify", "dpgo_problem_certify_device",
                 "dpgo_problem_certificate_apply", "dpgo_certify_escape_device"]:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    for s in ["dpgo_certify_params", "dpgo_certify_result", "DPGO_CERT_CERTIFIED", "DPGO_CERT_NOT_CERTIFIED",
              "DPGO_CERT_NOT_CONVERGED"]:
        assert s in hdr


def test_param_defaults_match_header():
    import dpgo_amd.lib as L
    hdr = open(os.path.join(ROOT, "include", "dpgo_hip.h")).read()
    body = hdr[hdr.index("typedef struct dpgo_certify_params"):]
    body = body[:body.index("} dpgo_certify_params;")]
    c = L.CertifyParamsC()
    L.load().dpgo_certify_params_default(C.byref(c))
    for field, _ in L.CertifyParamsC._fields_:
        m = re.search(r"\b%s;.*?default (\S+)" % field, body, re.S)
        assert m, field
        want = m.group(1)
        got = getattr(c, field)
        if want == "AUTO":
            assert got == L.PRECOND_AUTO
        else:
            assert got == pytest.approx(float(want), rel=0, abs=0), (field, got, want)


def _pose_graph(oracle, d, r, shared=False, prior=False):
    import dpgo_amd
    from conftest import to_product_measurements
    om, n = ref.ring_measurements(oracle, 16, d)
    if shared:  # edge 0 becomes an inter-robot loop closure: G != 0
        om.r2 = om.r2.copy()
        om.r2[0] = 1
    pg = dpgo_amd.PoseGraph(0, r, d)
    pg.setMeasurements(to_product_measurements(om))
    if prior:
        pg.setPrior(0, np.eye(r, d + 1))
    return pg


def test_python_mirror_rejects_bad_input_before_the_device(oracle):
    from dpgo_amd import certificate as cert
    pg = _pose_graph(oracle, 3, 3)
    n = pg.n()
    cert.check_certifiable(pg, np.zeros((3, 4 * n)))
    with pytest.raises(ValueError):
        cert.check_certifiable(pg, np.zeros((3, 4 * n + 1)))
    with pytest.raises(ValueError):
        cert.check_certifiable(pg, np.zeros((4, 4 * n)))
    with pytest.raises(ValueError):
        cert.check_certifiable(_pose_graph(oracle, 3, 3, prior=True))
    with pytest.raises(ValueError):
        cert.check_certifiable(_pose_graph(oracle, 3, 3, shared=True))
    with pytest.raises(ValueError):
        cert.check_certifiable(_pose_graph(oracle, 3, 7))  # (3, 7) is not compiled
    with pytest.raises(ValueError):
        cert.certify_params(tol_rel=0.0)
    with pytest.raises(ValueError):
        cert.certify_params(precond="cholesky")
    om, _ = ref.ring_measurements(oracle, 16, 3)
    from conftest import to_product_measurements
    with pytest.raises(ValueError):
        cert.solveCertifiedPGO(to_product_measurements(om), r0=2)
    with pytest.raises(ValueError):
        cert.solveCertifiedPGO(to_product_measurements(om), r0=7)


@pytest.mark.parametrize("d,r", [(2, 2), (2, 3), (3, 3), (3, 4)])
def test_ring_analytic_values_hold_for_the_restatement(oracle, d, r):
    om, n = ref.ring_measurements(oracle, 16, d)
    Q = ref.sparse_Q(oracle.construct_Q(n, d, om))
    lam = -2 * (1 - np.cos(2 * np.pi / 16))
    X1 = ref.ring_iterate(n, d, r, winding=1)
    Cm = ref.certificate_matrix(Q, X1, d).toarray()
    assert np.linalg.norm(X1 @ Cm) < 1e-12
    f = 0.5 * np.trace(X1 @ (Q @ X1.T))
    if d == 3:
        assert abs(f - 2.43585) < 1e-5
    w = np.linalg.eigvalsh(Cm)
    assert abs(w[0] - lam) < 1e-10 and abs(w[1] - lam) < 1e-10  # multiplicity 2
    assert abs(ref.complement_lambda_min(Cm, ref.null_basis(X1, d)) - lam) < 1e-10
    X0 = ref.ring_iterate(n, d, r, winding=0)
    C0 = ref.certificate_matrix(Q, X0, d).toarray()
    assert abs(0.5 * np.trace(X0 @ (Q @ X0.T))) < 1e-14
    Z = ref.null_basis(X0, d)
    assert Z.shape[1] == d + 1
    assert abs(ref.complement_lambda_min(C0, Z) + lam) < 1e-10
