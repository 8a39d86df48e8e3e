"""The certificate of global optimality on the device against tests/certificate_reference.py, case by case
(tests/certificate_cases.py; tests/test_certificate_cases_cpu.py holds the cases to their margins without a device).

Every handle is made on the C ABI from the oracle's own Q (dpgo_problem_set_Q_bsr), so the device and numpy see the same
matrix to the last bit.  Tolerances are derived (certificate_cases.check_pair), none is tuned: with w the returned witness,
lam the reported lambda_min, rho = |C w - lam w|_2 in numpy and eps = 1e-12 |C|_1,
  | |w| - 1 | <= 1e-10, |Z^T w| <= 1e-10, |w^T C w - lam| <= 1e-10 scale, a converged run has rho <= tol_rel scale + eps, and
  -eps <= lam - lam_ref <= rho + eps.
A run that ends NOT_CONVERGED, or stops on its budget, inside max(200, 4 x the restatement's count) iterations fails.
"""
import ctypes as C
import math

import numpy as np
import pytest

import certificate_cases as K
import certificate_reference as ref
from certificate_cases import DR, ETA, TOL_REL

pytestmark = pytest.mark.gpu

RTOL_ELEM = 1e-11  # (tests/test_parity_gpu.py)
_INST = {}


def _inst(key, make):
    if key not in _INST:
        _INST[key] = make()
    return _INST[key]


class Device:
    """A handle of rank r on an Instance's Q; closed on exit."""

    def __init__(self, inst, r=None):
        from test_launch_geometry_gpu import Handle
        import dpgo_amd.lib as L
        self.L, self.lib, self.inst = L, L.load(), inst
        self.h = Handle(self.lib, inst.Qb, inst.r if r is None else r, inst.d)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.h.close()

    def params(self, **kw):
        from dpgo_amd.certificate import certify_params
        return certify_params(**kw)

    def certify_rc(self, X, **kw):
        """(return code, CertificateResult, witness) of dpgo_problem_certify; the witness prefilled with NaN."""
        from dpgo_amd.certificate import CertificateResult
        cp, cr = self.params(**kw), self.L.CertifyResultC()
        Xc = np.asfortranarray(X, dtype=np.float64)
        w = np.full(X.shape[1], np.nan)
        rc = self.lib.dpgo_problem_certify(self.h.h, self.L.ptr(Xc), C.byref(cp), C.byref(cr), self.L.ptr(w))
        return rc, (CertificateResult.from_c(cr) if rc == self.L.OK else None), w

    def certify(self, X=None, **kw):
        rc, res, w = self.certify_rc(self.inst.X if X is None else X, **kw)
        self.L.check(rc)
        print("  %s lambda_min %.9e residual %.2e  %d its %d products  deflated %d (|C z| %.2e)  %.1f ms" % (
            res.status, res.lambda_min, res.residual, res.iterations, res.products, res.deflated, res.deflation_residual,
            res.elapsedMs))
        return res, w


def _finite(res, w):
    vals = [res.lambda_min, res.residual, res.gradnorm, res.scale, res.deflation_residual, res.elapsedMs]
    assert np.isfinite(vals).all() and np.isfinite(w).all(), (res, int(np.isnan(w).sum()))


def _check(oracle, inst, res, w, status, deflated, max_iterations, tol_rel=TOL_REL, eta=ETA, label=""):
    """A run that had to converge: status, deflated, scale, gradnorm, and the pair against numpy."""
    _finite(res, w)
    assert res.status == status, res
    assert res.deflated == deflated, res
    assert res.scale == inst.scale, (res.scale, inst.scale)  # a max: no rounding
    gn = inst.gradnorm(oracle)
    assert abs(res.gradnorm - gn) <= K.SCALAR_TOL * ref.operator_norm1(inst.Q) * np.linalg.norm(inst.X), (res.gradnorm, gn)
    assert res.residual <= tol_rel * res.scale and res.iterations < max_iterations, res  # converged inside the budget
    lam_ref = inst.lambda_ref(deflated)
    f = K.check_pair(inst, inst.Z(deflated), res.lambda_min, w, lam_ref, True, tol_rel, label)
    if status == "NOT_CERTIFIED":
        assert res.lambda_min < -eta * res.scale
    else:
        assert res.lambda_min >= -eta * res.scale
    return f


# ---------------------------------------------------------------- A
@pytest.mark.parametrize("d,r", DR)
def test_arbitrary_iterates(oracle, d, r):
    """Every (d, r) x {ragged, P - 1, P, P + 1, 17 P + 3} poses x {unit, random} weights at X = polar_project(Gaussian),
    precond = none: NOT_CERTIFIED with only t deflated; two cases again with block-Jacobi on the restatement's budget."""
    for c in [c for c in K.A_CASES if (c.d, c.r) == (d, r)]:
        inst = _inst(c, lambda: K.arbitrary(oracle, c))
        with Device(inst) as dev:
            its = K.budget(K.A_ITS)
            res, w = dev.certify(eta=ETA, tol_rel=TOL_REL, precond="none", max_iterations=its)
            _check(oracle, inst, res, w, "NOT_CERTIFIED", 1, its, label=c.name)
            if c in K.A_JACOBI:
                its = K.budget(K.A_JACOBI[c])
                resj, wj = dev.certify(eta=ETA, tol_rel=TOL_REL, precond="jacobi", max_iterations=its)
                _check(oracle, inst, resj, wj, "NOT_CERTIFIED", 1, its, label=c.name + " jacobi")


# ---------------------------------------------------------------- B
def _ring_both_windings(oracle, c, **over):
    prm = dict(K.RING_PARAMS, max_iterations=K.budget(K.RING_ITS[c.n]))
    prm.update(over)
    out = []
    for winding, status in ((1, "NOT_CERTIFIED"), (0, "CERTIFIED")):
        inst = _inst((c, winding), lambda: K.ring(oracle, c, winding))
        want = K.ring_lambda(c) if winding else -K.ring_lambda(c)
        assert abs(inst.lambda_ref(c.d + 1) - want) <= 1e-10 * inst.scale  # the dense reference and the formula
        with Device(inst) as dev:
            res, w = dev.certify(**prm)
        _check(oracle, inst, res, w, status, c.d + 1, prm["max_iterations"], label="%s winding %d" % (c.name, winding))
        assert abs(res.lambda_min - want) <= TOL_REL * inst.scale + 2 * inst.eps
        out.append(res)
    return out


@pytest.mark.parametrize("d,r", DR)
def test_twisted_rings(oracle, d, r):
    """Rings of P - 1, P + 1, 200 and 257 poses: lambda_min = -2 (1 - cos 2 pi / n) against the formula and the dense
    reference, d + 1 deflated directions; winding 0 is CERTIFIED at the smallest positive eigenvalue + |lambda_ring|."""
    for c in [c for c in K.B_CASES if (c.d, c.r) == (d, r)]:
        _ring_both_windings(oracle, c)


@pytest.mark.parametrize("c", K.B_SCALED, ids=lambda c: c.name)
def test_ring_scaled_weights(oracle, c):
    """kappa = tau = 7.5 on every edge: scale and lambda scale by 7.5, the same relative eta gives the same verdict."""
    one = K.Ring(c.d, c.r, c.n)
    a, b = _ring_both_windings(oracle, c), _ring_both_windings(oracle, one)
    for x, y in zip(a, b):
        assert x.status == y.status and x.scale == 7.5 * y.scale == 15.0
        bound = (TOL_REL * x.scale + 2 * _INST[(c, 1)].eps) + 7.5 * (TOL_REL * y.scale + 2 * _INST[(one, 1)].eps)
        assert abs(x.lambda_min - 7.5 * y.lambda_min) <= bound


@pytest.mark.parametrize("c", K.B_TURNED, ids=lambda c: c.name)
def test_ring_turned_iterate(oracle, c):
    """X replaced by A X (A orthogonal r x r): C is unchanged, no row of X is zero any more, and the rank-revealing cut has
    to find rank d + 1 by itself."""
    inst = _inst((c, 1), lambda: K.ring(oracle, c, 1))
    assert np.abs(inst.X).reshape(c.r, -1, c.d + 1)[:, :, :c.d].sum(axis=(1, 2)).min() > 1.0
    _ring_both_windings(oracle, c)


def test_ring_seeds_agree(oracle):
    c = K.B_SEEDED
    inst = _inst((c, 1), lambda: K.ring(oracle, c, 1))
    out = {}
    for seed in (1, 3, 12345):
        with Device(inst) as dev:
            its = K.budget(K.RING_ITS[c.n])
            res, w = dev.certify(**dict(K.RING_PARAMS, seed=seed, max_iterations=its))
        out[seed] = (res, _check(oracle, inst, res, w, "NOT_CERTIFIED", c.d + 1, its, label="seed %d" % seed))
    lams = [res.lambda_min for res, _ in out.values()]
    assert max(lams) - min(lams) <= max(f["rho"] for _, f in out.values()) + 2 * inst.eps


@pytest.mark.parametrize("c", K.B_PRECONDS, ids=lambda c: c.name)
def test_ring_preconditioners_agree(oracle, c):
    got = {pc: _ring_both_windings(oracle, c, precond=pc) for pc in ("jacobi", "multilevel")}
    for a, b in zip(got["jacobi"], got["multilevel"]):
        assert a.status == b.status and a.deflated == b.deflated
        assert abs(a.lambda_min - b.lambda_min) <= TOL_REL * a.scale + 2 * _INST[(c, 1)].eps


# ---------------------------------------------------------------- C
@pytest.mark.parametrize("c,eta,verdict", K.C_CASES, ids=lambda v: getattr(v, "name", str(v)))
def test_threshold_is_relative_and_two_sided(oracle, c, eta, verdict):
    """lambda / scale = -4.67e-3 (n = 65), -4.93e-4 (n = 200): CERTIFIED with a negative lambda_min above -eta scale at the
    larger eta, NOT_CERTIFIED at the smaller; no verdict within eta / 2 of the edge."""
    inst = _inst((c, 1), lambda: K.ring(oracle, c, 1))
    its = K.budget(K.RING_ITS[c.n])
    with Device(inst) as dev:
        res, w = dev.certify(**dict(K.RING_PARAMS, eta=eta, max_iterations=its))
    _check(oracle, inst, res, w, verdict, c.d + 1, its, eta=eta, label="%s eta %g" % (c.name, eta))
    assert res.lambda_min < 0


# ---------------------------------------------------------------- D
@pytest.mark.parametrize("c", K.D_CASES, ids=lambda c: type(c).__name__ + "-" + c.name)
def test_not_certified_is_a_proof_when_the_budget_ends(oracle, c):
    """max_iterations 1, 2, 5 (the restatement needs more on every case): whatever comes back is finite; NOT_CERTIFIED comes
    with a unit witness orthogonal to Z whose Rayleigh quotient in numpy is the reported lambda_min < -eta scale and not
    below lambda_ref; anything else is NOT_CONVERGED."""
    ring = isinstance(c, K.Ring)
    inst = _inst((c, 1), lambda: K.ring(oracle, c, 1)) if ring else _inst(c, lambda: K.arbitrary(oracle, c))
    k = c.d + 1 if ring else 1
    for its in K.D_BUDGETS:
        with Device(inst) as dev:
            res, w = dev.certify(eta=ETA, tol_rel=TOL_REL, precond="jacobi" if ring else "none", max_iterations=its, seed=3)
        _finite(res, w)
        assert res.iterations <= its and res.deflated == k
        if res.status == "NOT_CERTIFIED":
            K.check_pair(inst, inst.Z(k), res.lambda_min, w, inst.lambda_ref(k), False, label="%s budget %d" % (c.name, its))
            assert res.lambda_min < -ETA * res.scale, res
        else:
            assert res.status == "NOT_CONVERGED", res


# ---------------------------------------------------------------- E
@pytest.mark.parametrize("c", K.E_CASES, ids=lambda c: c.name)
def test_deflation_follows_the_documented_rule(oracle, c):
    """The ring iterate moved by eps along a fixed tangent vector: where every direction of its row space has
    |C z| >= 10 null_tol only t is deflated, where every one has |C z| <= null_tol / 10 all d + 1 are; deflation_residual
    is numpy's largest |C z| among the deflated directions; lambda_min is the reference's on the complement of exactly
    that.  (Between the two the rule decides by round-off: not tested.)"""
    inst = _inst(c, lambda: K.perturbed(oracle, c))
    its = K.budget(K.E_ITS)
    with Device(inst) as dev:
        res, w = dev.certify(eta=ETA, tol_rel=TOL_REL, precond="jacobi", max_iterations=its, seed=3)
    want = 0.0 if c.deflated == 1 else float(inst.row_space_residuals()[-1])
    print("  deflation_residual %.6e numpy %.6e (eps %.1e)" % (res.deflation_residual, want, inst.eps))
    _check(oracle, inst, res, w, "NOT_CERTIFIED", c.deflated, its, label=c.name)
    assert abs(res.deflation_residual - want) <= inst.eps


# ---------------------------------------------------------------- F
@pytest.mark.parametrize("c", K.F_CASES, ids=lambda c: c.name)
def test_big_blocks(oracle, c):
    """Second trips of the grid-stride loops (kBlock = 256, kMaxGrid = kPartialCap = 1024 of kernels/common.h; kCertCols =
    64 of kernels/certify.h; Cert::kGramWg = 512 of certify.hip), at an arbitrary X with precond = none:
      2-D lattice 110 x 100, r = 3: 33 000 columns = 516 chunks of 64 > 512 workgroups -- workgroups 0 .. 3 of k_cert_gram
        take a second trip of the chunk loop, and the last chunk holds 40 columns (base + e < total).
      synthetic_grid(21, 21, 21), r = 4: 37 044 columns = 579 chunks -- 67 workgroups of k_cert_gram repeat, d = 3.
      synthetic_grid(41, 41, 40), r = 5: 67 240 poses = 1 051 tiles of 64 > the launch cap 1 024 of k_cert_apply (27
        workgroups take a second tile, plain and symmetric storage alike); 268 960 columns = 4 203 chunks, eight or nine
        trips of k_cert_gram per workgroup; 1 051 blocks of 256 columns > 1 024, so 27 workgroups of k_cert_combine (and
        of k_cert_indicator) repeat their column loop; k_cert_reduce sums 512 partials per Gram entry and 1 024 for
        w^T C w.  The smallest size at which k_cert_combine repeats.  Run on the plain and on the symmetric storage of Q
        (Cert::sym): both against the reference, and within the bound of each other.
    Each size also runs with max_iterations = 2: the eigenvector of C at a random X is localised, so a converged witness
    does not notice a Gram sum that loses a few hundred of these columns (k_cert_gram stopping one chunk early passed
    the converged checks), while after two iterations w still lives on every column, and a lost chunk shows in |w| and
    in w^T t.  Whatever the status then, the witness is unit, orthogonal to t, and lambda_min its Rayleigh quotient."""
    inst = _inst(c, lambda: K.big(oracle, c))
    if (1, 2) not in inst._ref:  # eigsh(C, k = 1, which = "SA", tol = 1e-12), once per module
        inst._ref[(1, 2)] = K.big_lambdas(inst, 1)
    its = K.budget(c.its)
    got = []
    for variant in c.variants:
        with Device(inst) as dev:
            if variant != "auto":
                code, v = {"plain": 1, "symmetric": 2}[variant], C.c_int(0)
                dev.L.check(dev.lib.dpgo_problem_set_spmm_variant(dev.h.h, code, C.byref(v)))
                assert v.value == code
            early, we = dev.certify(eta=ETA, tol_rel=TOL_REL, precond="none", max_iterations=2)
            res, w = dev.certify(eta=ETA, tol_rel=TOL_REL, precond="none", max_iterations=its)
        _finite(early, we)
        K.check_pair(inst, inst.Z(1), early.lambda_min, we, inst.lambda_ref(1), False, label="%s %s budget 2" % (c.name, variant))
        assert early.status in ("NOT_CERTIFIED", "NOT_CONVERGED") and early.deflated == 1
        got.append((res, _check(oracle, inst, res, w, "NOT_CERTIFIED", 1, its, label="%s %s" % (c.name, variant))))
    if len(got) == 2:
        (a, fa), (b, fb) = got
        assert abs(a.lambda_min - b.lambda_min) <= max(fa["rho"], fb["rho"]) + 2 * inst.eps


# ---------------------------------------------------------------- G
def _scalars(cr):
    return [getattr(cr, name) for name, _ in type(cr)._fields_ if name != "elapsedMs"]


@pytest.mark.parametrize("c", [K.Arbitrary(3, 4, 65, False), K.Ring(2, 3, 85)], ids=lambda c: type(c).__name__ + "-" + c.name)
def test_device_entry_is_bitwise_the_host_entry(oracle, c):
    """dpgo_problem_certify_device on torch buffers: status, every scalar and the witness are bitwise those of
    dpgo_problem_certify; the strided witness copy writes exactly (d+1)n doubles between its guards; witness_dev = NULL."""
    import torch
    from test_launch_geometry_gpu import Guarded, guard_of
    ring = isinstance(c, K.Ring)
    inst = _inst((c, 1), lambda: K.ring(oracle, c, 1)) if ring else _inst(c, lambda: K.arbitrary(oracle, c))
    prm = dict(eta=ETA, tol_rel=TOL_REL, precond="jacobi" if ring else "none", seed=3,
               max_iterations=K.budget(K.RING_ITS[c.n] if ring else K.A_ITS))
    N = inst.X.shape[1]
    with Device(inst) as dev:
        L, lib = dev.L, dev.lib
        cp = dev.params(**prm)
        host, w = L.CertifyResultC(), np.full(N, np.nan)
        Xc = np.asfortranarray(inst.X)
        L.check(lib.dpgo_problem_certify(dev.h.h, L.ptr(Xc), C.byref(cp), C.byref(host), L.ptr(w)))
        Xd = torch.from_numpy(K.tiles_of(inst.X, inst.d).copy()).to("cuda")
        torch.cuda.synchronize()
        out = Guarded(N, guard_of(inst.d, inst.r), device=True)
        a, b = L.CertifyResultC(), L.CertifyResultC()
        L.check(lib.dpgo_problem_certify_device(dev.h.h, L.ptr(Xd), C.byref(cp), C.byref(a), out.ptr()))
        wd = out.result((N,))
        L.check(lib.dpgo_problem_certify_device(dev.h.h, L.ptr(Xd), C.byref(cp), C.byref(b), None))
    assert _scalars(a) == _scalars(host) == _scalars(b), (_scalars(a), _scalars(host), _scalars(b))
    assert a.status == L.CERT_NOT_CERTIFIED
    assert np.array_equal(wd, w)
    K.check_pair(inst, inst.Z(c.d + 1 if ring else 1), a.lambda_min, wd, inst.lambda_ref(c.d + 1 if ring else 1), True,
                 label=c.name)


@pytest.mark.parametrize("d,r", K.LIFTS)
def test_escape_lifts_and_retracts(oracle, d, r):
    """dpgo_certify_escape_device for every r -> r + 1 on rings of P + 1 and 257 poses: with the returned alpha, X_next is
    oracle.qf_retract of [X; alpha w^T] (zero step) to RTOL_ELEM; Y^T Y = I to 1e-12; f(X_next) < f(X) by the oracle;
    alpha = 0.1 sqrt(n) 2^-k for an integer 0 <= k < 60 (which k is not asserted); a handle of the wrong rank is
    DPGO_ERR_INVALID."""
    import torch
    for n in (K.tile_poses(d) + 1, 257):
        c = K.Ring(d, r, n)
        inst = _inst((c, 1), lambda: K.ring(oracle, c, 1))
        N = inst.X.shape[1]
        with Device(inst) as dev, Device(inst, r + 1) as nxt:
            L, lib = dev.L, dev.lib
            cp = dev.params(**dict(K.RING_PARAMS, max_iterations=K.budget(K.RING_ITS[n])))
            Xd = torch.from_numpy(K.tiles_of(inst.X, d).copy()).to("cuda")
            wd = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
            Xn = torch.full((N, r + 1), float("nan"), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            cr = L.CertifyResultC()
            L.check(lib.dpgo_problem_certify_device(dev.h.h, L.ptr(Xd), C.byref(cp), C.byref(cr), L.ptr(wd)))
            assert cr.status == L.CERT_NOT_CERTIFIED
            alpha = C.c_double(-1.0)
            rc = lib.dpgo_certify_escape_device(dev.h.h, r, L.ptr(Xd), L.ptr(wd), 1e-9, L.ptr(Xn), C.byref(alpha))
            assert rc == L.ERR_INVALID  # a handle of rank r, not r + 1
            L.check(lib.dpgo_certify_escape_device(nxt.h.h, r, L.ptr(Xd), L.ptr(wd), 1e-9, L.ptr(Xn), C.byref(alpha)))
            torch.cuda.synchronize()
            got, w = Xn.cpu().numpy().reshape(n, d + 1, r + 1), wd.cpu().numpy()
        a = alpha.value
        ratio = 0.1 * math.sqrt(n) / a
        k = round(math.log2(ratio))
        print("  %s -> r + 1: alpha %.6e = 0.1 sqrt(n) 2^-%d" % (c.name, a, k))
        assert a > 0 and 0 <= k < 60 and ratio == 2.0 ** k, (a, ratio)
        lifted = np.concatenate([K.tiles_of(inst.X, d), a * w.reshape(n, d + 1, 1)], axis=2)
        want = oracle.qf_retract(lifted, np.zeros_like(lifted), d)
        assert np.isfinite(got).all()
        assert np.abs(got - want).max() <= RTOL_ELEM * np.abs(want).max(), np.abs(got - want).max()
        Y = got[:, :d, :]
        assert np.abs(Y @ np.swapaxes(Y, 1, 2) - np.eye(d)).max() <= 1e-12
        f = oracle.QuadraticProblem(inst.Qb, None, r + 1, d, precond="none").f
        f0, f1 = f(np.concatenate([K.tiles_of(inst.X, d), np.zeros((n, d + 1, 1))], axis=2)), f(got)
        print("  f %.12e -> %.12e" % (f0, f1))
        assert f1 < f0


# ---------------------------------------------------------------- H
@pytest.mark.parametrize("d,r,n,start", K.H_CASES)
def test_tiny_graphs_never_get_a_wrong_verdict(oracle, d, r, n, start):
    """Chains of 1, 2, 3 and 5 poses at a random X and at the noiseless truth: the call returns an error code or a status,
    every output is finite, and a CERTIFIED or NOT_CERTIFIED verdict agrees with the dense reference on the complement of
    what the documented rule deflates.

    What the library does with m = (d+1)n - dim Z directions left (include/dpgo_hip.h says so): m < r is DPGO_ERR_STATE
    (the start block is rank deficient: n = 1 at r = 5; two 2-D or 3-D poses at the truth and r = 5); m = r gives the exact
    pair at iteration 0; r < m < 3r stops on a dependent basis after 0 - 2 iterations, NOT_CERTIFIED with a valid,
    unconverged witness at a random X and NOT_CONVERGED at the truth; from m = 3r on (three 2-D poses at r = 2) it
    converges, CERTIFIED at the truth."""
    inst = K.tiny(oracle, d, r, n, start)
    with Device(inst) as dev:
        rc, res, w = dev.certify_rc(inst.X, eta=ETA, tol_rel=TOL_REL, precond="jacobi", max_iterations=200, seed=3)
    N, (Z, clear) = inst.C.shape[0], inst.documented_Z()
    print("  N %d dim Z %d (3 r = %d): rc %d %s" % (N, Z.shape[1], 3 * r, rc, res))
    assert rc in (dev.L.OK, dev.L.ERR_INVALID, dev.L.ERR_STATE, dev.L.ERR_UNSUPPORTED)
    if rc != dev.L.OK:
        return
    vals = [res.lambda_min, res.residual, res.gradnorm, res.scale, res.deflation_residual]
    assert np.isfinite(vals).all(), res
    if res.status == "NOT_CONVERGED" or not clear:
        return
    assert np.isfinite(w).all() and res.deflated == Z.shape[1] < N, res
    lam_ref = float(ref.lambda_min_dense(inst.C, Z)[0])
    K.check_pair(inst, Z, res.lambda_min, w, lam_ref, res.status == "CERTIFIED", label="tiny")
    if res.status == "NOT_CERTIFIED":
        assert res.lambda_min < -ETA * res.scale and lam_ref < -ETA * res.scale
    else:
        assert lam_ref >= -ETA * res.scale - inst.eps, (res, lam_ref)
