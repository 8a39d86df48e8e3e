"""The case table of tests/certificate_cases.py is complete and every case of it is fit for what
tests/test_certificate_cases_gpu.py asserts -- on the reference alone (no GPU).

For every case: the dense and the Lanczos route to lambda_min agree to 1e-10 scale where both are affordable; the numpy
restatement of the documented iteration converges to lambda_ref within the derived bound (certificate_cases.check_pair)
and within the recorded count that the device's budget is four times of; groups A and F keep a gap
(lambda_2 - lambda_1) / scale >= 1e-3; the margins of groups C, D and E hold; and whether X counts as stationary
(|C z| over the row space of X against null_tol = sqrt(tol_rel) scale) is a factor 10 from the threshold at least.  These
are conditions on the INPUTS: a case that misses one gets another seed (certificate_cases.SEEDS), never a looser assertion.
"""
import numpy as np
import pytest

import certificate_cases as K
import certificate_reference as ref
from certificate_cases import DR, TOL_REL


def test_tables_are_complete():
    for d, r in DR:
        P = K.tile_poses(d)
        a = [c for c in K.A_CASES if (c.d, c.r) == (d, r)]
        assert {(c.n, c.unit) for c in a} == {(n, u) for n in (K.RAGGED[d], P - 1, P, P + 1, 17 * P + 3) for u in (True, False)}
        cols = (d + 1) * K.RAGGED[d]
        assert cols % 64 != 0 and 64 < cols <= 64 + (d + 1)  # the shortest second chunk a pose count can give
        assert {c.n for c in K.B_CASES if (c.d, c.r) == (d, r)} == {P - 1, P + 1, 200, 257}
        assert sum((c.d, c.r) == (d, r) for c in K.D_CASES) == 2
    assert K.LIFTS == [(2, 2), (2, 3), (2, 4), (3, 3), (3, 4), (3, 5)]
    assert set(K.SEEDS) <= set(K.A_CASES) and set(K.A_JACOBI) <= set(K.A_CASES)
    assert {c.n for c in K.B_CASES + K.B_SCALED + K.B_TURNED + K.B_PRECONDS + [K.B_SEEDED]} <= set(K.RING_ITS)
    assert any(c.r > c.d for c in K.B_TURNED)  # the zero rows of the ring iterate are what turning removes
    assert [c.dims for c in K.F_CASES] == ["110x100", "21x21x21", "41x41x40"] and [c.r for c in K.F_CASES] == [3, 4, 5]
    assert K.budget(K.A_ITS) == 200 and K.budget(K.RING_ITS[257]) == 4 * K.RING_ITS[257]


def test_reference_routes_agree(oracle):
    """eigvalsh of the projected matrix, eigsh(which="SA") of the projected operator and the SVD-based
    complement_lambda_min, on an arbitrary iterate (Z = t) and on a ring (Z = rows of X and t)."""
    for inst, k in [(K.arbitrary(oracle, K.Arbitrary(3, 4, 63, False)), 1), (K.arbitrary(oracle, K.Arbitrary(2, 5, 85, True)), 1),
                    (K.ring(oracle, K.Ring(3, 5, 65)), 4), (K.ring(oracle, K.Ring(2, 2, 83), winding=0), 3)]:
        Z = inst.Z(k)
        dense = ref.lambda_min_dense(inst.C, Z, 2)
        assert abs(dense[0] - ref.complement_lambda_min(inst.C.toarray(), Z)) <= 1e-10 * inst.scale
        if k == 1:  # (the ring's smallest eigenvalue is double and 1e-3 scale from the next: Lanczos is the wrong tool)
            assert np.abs(ref.lambda_min_lanczos(inst.C, Z, 2) - dense).max() <= 1e-10 * inst.scale
            # C t = 0 exactly and lambda_min < 0: no projection is needed at all
            assert abs(np.linalg.eigvalsh(inst.C.toarray())[0] - dense[0]) <= 1e-10 * inst.scale
            assert np.abs(inst.C @ Z).max() <= 1e-13 * inst.scale


def _restated(inst, Z, r, lam_ref, limit, precond=None, label=""):
    its, theta, w, ok = K.restatement(inst.C, Z, r, TOL_REL * inst.scale, precond=precond, max_iterations=limit)
    assert ok and 5 < its <= limit, (label, its, limit)
    K.check_pair(inst, Z, theta, w, lam_ref, True, label=label)
    return its


@pytest.mark.parametrize("d,r", DR)
def test_arbitrary_iterates(oracle, d, r):
    for c in [c for c in K.A_CASES if (c.d, c.r) == (d, r)]:
        inst = K.arbitrary(oracle, c)
        lam = inst.lambdas(1, 2)
        assert lam[0] < -1e-2 * inst.scale, c.name  # strongly indefinite: NOT_CERTIFIED at any sensible eta
        assert (lam[1] - lam[0]) >= K.GAP * inst.scale, c.name
        assert inst.row_space_residuals()[0] >= 10 * inst.null_tol(), c.name  # only t is deflated
        assert inst.scale == np.max(inst.Q.diagonal())
        _restated(inst, inst.Z(1), r, lam[0], K.A_ITS, label=c.name)  # (more than 5: group D's budgets end first)
        if c in K.A_JACOBI:
            _restated(inst, inst.Z(1), r, lam[0], K.A_JACOBI[c], precond=inst.jacobi(), label=c.name + " jacobi")


@pytest.mark.parametrize("d,r", DR)
def test_rings(oracle, d, r):
    cases = [c for c in K.B_CASES + K.B_SCALED + K.B_TURNED if (c.d, c.r) == (d, r)]
    for c in cases:
        for winding in (1, 0):
            inst = K.ring(oracle, c, winding)
            Z = inst.Z(d + 1)
            lam = inst.lambda_ref(d + 1)
            want = K.ring_lambda(c) if winding else -K.ring_lambda(c)
            assert abs(lam - want) <= 1e-10 * inst.scale, c.name
            assert inst.scale == 2.0 * c.kappa
            assert inst.row_space_residuals()[-1] <= 0.1 * inst.null_tol(), c.name  # stationary: d + 1 deflated
            assert abs(lam / inst.scale + K.ETA) >= 0.5 * K.ETA
            _restated(inst, Z, r, lam, K.RING_ITS[c.n], label="%s winding %d" % (c.name, winding))
            if c in K.B_PRECONDS:
                _restated(inst, Z, r, lam, K.RING_ITS[c.n], precond=inst.jacobi(), label=c.name + " jacobi")


def test_threshold_cases_are_off_the_edge(oracle):
    for c, eta, verdict in K.C_CASES:
        inst = K.ring(oracle, c)
        ratio = inst.lambda_ref(c.d + 1) / inst.scale
        assert abs(ratio + eta) >= 0.5 * eta, (c.name, eta)
        assert (ratio < -eta) == (verdict == "NOT_CERTIFIED"), (c.name, eta)
        assert ratio < 0
    assert {v for _, _, v in K.C_CASES} == {"CERTIFIED", "NOT_CERTIFIED"}


def test_budget_cases_need_more_than_five_iterations(oracle):
    for c in K.D_CASES:
        ring = isinstance(c, K.Ring)
        inst = K.ring(oracle, c) if ring else K.arbitrary(oracle, c)
        k = c.d + 1 if ring else 1
        its = K.restatement(inst.C, inst.Z(k), c.r, TOL_REL * inst.scale)[0]
        assert its > max(K.D_BUDGETS), (c.name, its)
        assert inst.lambda_ref(k) < -K.ETA * inst.scale


def test_deflation_cases_are_a_factor_ten_from_the_rule(oracle):
    for c in K.E_CASES:
        inst = K.perturbed(oracle, c)
        res = inst.row_space_residuals()
        assert len(res) == c.d
        if c.deflated == 1:
            assert res[0] >= 10 * inst.null_tol(), (c.name, res / inst.null_tol())
        else:
            assert c.deflated == c.d + 1 and res[-1] <= 0.1 * inst.null_tol(), (c.name, res / inst.null_tol())
        Z, clear = inst.documented_Z()
        assert clear and Z.shape[1] == c.deflated
        lam = inst.lambda_ref(c.deflated)
        assert lam < -K.ETA * inst.scale
        _restated(inst, inst.Z(c.deflated), c.r, lam, K.E_ITS, label=c.name)


@pytest.mark.parametrize("c", K.F_CASES, ids=lambda c: c.name)
def test_big_blocks(oracle, c):
    inst = K.big(oracle, c)
    lam = K.big_lambdas(inst, 2)
    assert lam[0] < -1e-2 * inst.scale and lam[1] - lam[0] >= K.GAP * inst.scale
    assert np.abs(inst.C @ inst.Z(1)).max() <= 1e-13 * inst.scale
    if c in K.F_RESTATED:
        _restated(inst, inst.Z(1), c.r, lam[0], c.its, label=c.name)
        assert abs(ref.lambda_min_lanczos(inst.C, inst.Z(1))[0] - lam[0]) <= 1e-10 * inst.scale
    else:  # the count of the nearest smaller case of the same family
        assert c.its == K.F_CASES[1].its and K.F_CASES[1] in K.F_RESTATED


def test_tiny_cases_have_a_dense_reference(oracle):
    for d, r, n, start in K.H_CASES:
        inst = K.tiny(oracle, d, r, n, start)
        assert inst.C.shape[0] == (d + 1) * n <= 20
        Z, clear = inst.documented_Z()
        if clear and Z.shape[1] < inst.C.shape[0]:
            assert np.isfinite(ref.lambda_min_dense(inst.C, Z)[0])
