"""tests/team_staircase_reference.py pinned on the 16-pose identity ring at the winding-1 saddle (no GPU): the figures the
GPU tests of the team staircase rest on.  f = 2.435855 = 16 (1 - cos 2 pi / 16) 2, |rgrad| at rounding,
lambda_min = -2 (1 - cos 2 pi / 16); the first trial step alpha0 = 0.1 sqrt(16) is accepted with f_after = 2.423796."""
import numpy as np
import pytest

import certificate_cases as K
import certificate_reference as ref
import team_staircase_reference as tsr

LAM_RING = -2.0 * (1.0 - np.cos(2.0 * np.pi / 16))


@pytest.mark.parametrize("d", [2, 3])
def test_reference_on_the_twisted_ring(oracle, d):
    om, Qb, Qs = K.ring_graph(oracle, d, 16)
    X = ref.ring_iterate(16, d, d, 1)
    f, rg, S = tsr.team_eval(Qs, X, d)
    lam, w = tsr.dense_witness(Qs, X, d)
    print("d = %d: f %.9f  |rgrad| %.2e  lambda_min %.9f" % (d, f, np.linalg.norm(rg), lam))
    assert abs(f - 2.435855) <= 1e-6
    assert abs(f - oracle.QuadraticProblem(Qb, None, d, d, precond="none").f(K.tiles_of(X, d))) <= 1e-12 * f
    assert np.linalg.norm(rg) <= 1e-12
    assert np.allclose(rg, K.matrix_of(oracle.QuadraticProblem(Qb, None, d, d, precond="none").rie_grad(K.tiles_of(X, d))),
                       atol=1e-13)
    assert S.shape == (16, d, d) and np.allclose(S, S.transpose(0, 2, 1))
    assert abs(lam - LAM_RING) <= 1e-9 and abs(lam + 0.1522409) <= 1e-7
    e = tsr.escape(oracle, Qs, X, w, d, 1e-6)
    print("  escape: k %d alpha %.3f  f %.6f -> %.6f  |rgrad| %.2e" % (e["k"], e["alpha"], e["f_before"], e["f_after"],
                                                                      e["gradnorm_after"]))
    assert e["k"] == 0 and e["alpha"] == 0.1 * np.sqrt(16)
    assert e["f_before"] == f
    assert abs(e["f_after"] - 2.423796) <= 1e-6
    assert abs(e["gradnorm_after"] - 6.0e-2) <= 0.5e-2
    Xn = e["X"]
    assert Xn.shape == (d + 1, (d + 1) * 16)
    Y = K.tiles_of(Xn, d)[:, :d, :]
    assert np.abs(Y @ Y.transpose(0, 2, 1) - np.eye(d)).max() <= 1e-14


def test_reference_rgrad_at_a_random_iterate(oracle):
    """team_eval against the oracle's QuadraticProblem where the gradient is nowhere near zero."""
    d, r, n = 3, 5, 23
    om, Qb, Qs = K.random_graph(oracle, d, n, False)
    X = K.random_iterate(oracle, n, d, r, 7)
    f, rg, _ = tsr.team_eval(Qs, X, d)
    qp = oracle.QuadraticProblem(Qb, None, r, d, precond="none")
    assert abs(f - qp.f(K.tiles_of(X, d))) <= 1e-13 * abs(f)
    want = K.matrix_of(qp.rie_grad(K.tiles_of(X, d)))
    assert np.linalg.norm(rg - want) <= 1e-13 * np.linalg.norm(want)


def test_team_staircase_symbols_are_exported():
    import dpgo_amd.lib as L
    lib = L.load()
    for name in ("dpgo_team_eval_device", "dpgo_team_escape_device"):
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    import dpgo_amd
    assert callable(dpgo_amd.solveCertifiedDistributedPGO)
    from dpgo_amd.certificate import escape_team, evaluate_team  # noqa: F401
