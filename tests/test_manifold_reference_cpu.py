"""tests/manifold_reference.py checked on its own (CPU only): the longdouble polar factor, rotation, rounding and qf
retraction are orthonormal to longdouble round-off, agree with mpmath at 50 digits, and bound the error of the oracle's
fp64 restatements by 64 eps kappa in every condition class.  The NumPy emulations of the two routes a kernel can take to
U V^T are kept here as the witness of why kernels/manifold.h factors M itself: through the Gram matrix M^T M the result
loses eps kappa^2, by one-sided Jacobi on M it stays orthonormal to round-off up to kappa = 1e12."""
import numpy as np
import pytest

try:
    import manifold_reference as MR
except AssertionError as e:  # np.longdouble is plain fp64 on this platform
    pytest.skip(str(e), allow_module_level=True)

LD = MR.LD


def _orth_err(Y):
    """max |Y Y^T - I| of tiles' rotation rows Y [n, d, r] (= Y^T Y of the r x d blocks)."""
    d = Y.shape[1]
    return float(np.abs(Y @ np.swapaxes(Y, 1, 2) - np.eye(d, dtype=Y.dtype)).max())


@pytest.fixture(scope="module")
def polar_refs():
    """{(d, r): (M, cls, polar_ld(M))} at n = 333, computed once."""
    out = {}
    for d, r in MR.DR:
        M, cls = MR.polar_cases(d, r, 333)
        out[d, r] = (M, cls, MR.polar_ld(M))
    return out


@pytest.fixture(scope="module")
def round_refs():
    out = {}
    for d, r in MR.DR:
        X, anchor, cls, refl = MR.round_cases(d, r, 333)
        out[d, r] = (X, anchor, cls, refl, MR.round_ld(X, d), MR.round_ld(X, d, anchor))
    return out


def test_generators_build_the_stated_classes():
    for n in MR.SIZES:
        cls, sci = MR.pose_classes(n)
        assert len(cls) == n and cls[0] == 0
    cls, sci = MR.pose_classes(333)
    counts = np.bincount(cls, minlength=MR.NCLASS)
    assert counts.min() >= 15 and counts.max() <= 16
    for c in range(MR.NCLASS):  # a class moves through the lanes and meets every scale
        assert len(set(np.nonzero(cls == c)[0] % 16)) >= 14 and len(set(np.nonzero(cls == c)[0] % 21)) >= 15
        assert set(sci[cls == c]) == {0, 1, 2}
    for d, r in MR.DR:
        M, cls = MR.polar_cases(d, r, 333)
        s = np.linalg.svd(M[:, :d, :], compute_uv=False)
        kap = s[:, 0] / s[:, -1]
        assert np.abs(kap / MR.class_kappa(cls) - 1).max() < 1e-3  # (the blocks are built in fp64: eps kappa)
        assert set(np.round(np.log10(s[:, 0])).astype(int)) == {-8, 0, 8}
        X, anchor, cls, refl = MR.round_cases(d, r, 333)
        for A in (X[0], anchor):
            Mb = np.einsum("ak,nbk->nab", A[:d], X[:, :d])
            assert ((np.linalg.det(Mb) < 0) == refl).all()
        assert 0.2 < refl.mean() < 0.3
        assert (cls[refl] % 3 == 0).all() and (cls[refl] >= 3).all()  # geometric spectra with kappa > 1 only


def test_reference_is_orthonormal_in_longdouble(polar_refs, round_refs):
    for (d, r), (M, cls, ref) in polar_refs.items():
        assert ref.dtype == LD
        assert _orth_err(ref[:, :d, :]) <= 1e-17, (d, r)
        assert (ref[:, d, :] == M[:, d, :]).all()
    for (d, r), (X, anchor, cls, refl, T0, Ta) in round_refs.items():
        for T in (T0, Ta):
            assert _orth_err(T[:, :d, :]) <= 1e-17, (d, r)
            assert float(np.abs(MR._det(T[:, :d, :]) - 1).max()) <= 1e-17, (d, r)
    for d, r in MR.DR:
        X, eta, cls = MR.retraction_cases(d, r, 17)
        Q = MR.qf_ld(X, eta, 1.0)
        assert _orth_err(Q[:, :d, :]) <= 1e-17
        # the positive-diagonal R: q_k . a_k > 0, and a_0 is parallel to q_0
        A = (MR._ld(X) + MR._ld(eta))[:, :d, :]
        assert (np.sum(Q[:, :d, :] * A, axis=2) > 0).all()
        c0 = np.sum(Q[:, 0, :] * A[:, 0, :], axis=1) / np.sqrt(np.sum(A[:, 0, :] ** 2, axis=1))
        assert float(np.abs(c0 - 1).max()) <= 1e-17


def _mp_polar(mp, A, rotation):
    """U V^T of the SVD of A (a list-of-rows matrix) at mpmath precision; the last column of U negated when
    `rotation` and det U det V < 0."""
    U, S, Vt = mp.svd_r(mp.matrix(A))
    if rotation and mp.det(U) * mp.det(Vt) < 0:
        for i in range(U.rows):
            U[i, U.cols - 1] = -U[i, U.cols - 1]
    return U * Vt


def test_reference_agrees_with_mpmath(polar_refs, round_refs):
    """Four blocks of every class of every (d, r) against mpmath at 50 digits.  Both take the exact polar factor of the
    same fp64 block, so the difference is this module's own error: 2^-64 times the factor's condition number, at most
    kappa; 64 of those are allowed."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    u = float(np.finfo(LD).eps)
    for (d, r), (M, cls, ref) in polar_refs.items():
        for c in range(MR.NCLASS):
            for i in np.nonzero(cls == c)[0][:4]:
                A = M[i, :d, :].T  # r x d
                P = _mp_polar(mp, [[mp.mpf(float(v)) for v in row] for row in A], False)
                err = max(abs(P[a, b] - mp.mpf(str(ref[i, b, a]))) for a in range(r) for b in range(d))
                assert err <= 64 * u * MR.KAPPAS[c // 3] + 1e-18, (d, r, MR.class_name(c), i, float(err))
    for (d, r), (X, anchor, cls, refl, T0, Ta) in round_refs.items():
        for c in range(MR.NCLASS):
            idx = np.nonzero(cls == c)[0]
            for i in list(idx[:2]) + list(idx[refl[idx]][:2]):
                for A, T in ((X[0], T0), (anchor, Ta)):
                    Ya = mp.matrix([[mp.mpf(float(v)) for v in row] for row in A[:d]])       # d x r = Ya^T
                    Yi = mp.matrix([[mp.mpf(float(v)) for v in row] for row in X[i, :d]]).T  # r x d
                    Mm = Ya * Yi
                    P = _mp_polar(mp, Mm, True)
                    # for a reflected block the nearest rotation moves by |dM| / (s_{d-1} - s_d)
                    s = sorted([float(v) for v in mp.svd_r(Mm, compute_uv=False)])
                    cond = s[-1] / ((s[1] - s[0]) if refl[i] else (s[1] + s[0]) / 2)
                    err = max(abs(P[a, b] - mp.mpf(str(T[i, b, a]))) for a in range(d) for b in range(d))
                    assert err <= 64 * u * cond + 1e-18, (d, r, MR.class_name(c), i, float(err), cond)
                    p = mp.matrix([mp.mpf(float(v)) for v in X[i, d]])
                    pa = mp.matrix([mp.mpf(float(v)) for v in A[d]])
                    tt = Ya * p - Ya * pa
                    mag = max(abs(v) for v in Ya * p) + max(abs(v) for v in Ya * pa)
                    assert max(abs(tt[a] - mp.mpf(str(T[i, d, a]))) for a in range(d)) <= 64 * u * mag


def test_fp64_restatements_stay_within_eps_kappa(oracle, polar_refs, round_refs):
    """oracle.polar_project / oracle.round_trajectory (LAPACK SVD in fp64) against the reference: element errors within
    64 eps kappa in every class -- the yardstick the device is held to lies where fp64 can reach."""
    for (d, r), (M, cls, ref) in polar_refs.items():
        E = MR.per_class_max(np.abs(oracle.polar_project(M, d) - ref)[:, :d], cls)
        for c, e in E.items():
            assert e <= 64 * MR.EPS * MR.KAPPAS[c // 3], (d, r, MR.class_name(c), e)
    for (d, r), (X, anchor, cls, refl, T0, Ta) in round_refs.items():
        for A, T in ((None, T0), (anchor, Ta)):
            E = MR.per_class_max(np.abs(oracle.round_trajectory(X, d, A) - T)[:, :d], cls)
            for c, e in E.items():
                assert e <= 64 * MR.EPS * MR.KAPPAS[c // 3], (d, r, MR.class_name(c), e)


def test_qf_reference_bounds_the_oracles_gram_schmidt(oracle):
    """oracle.qf_retract (modified Gram-Schmidt, the same recurrence as the device's qf_col) against the Householder
    reference at step norms 1, 1e2 and 1e4: a point plus a step of norm s has kappa <= 1 + s."""
    for d, r in MR.DR:
        X, eta, cls = MR.retraction_cases(d, r, 17)
        err = MR.per_class_max(np.abs(oracle.qf_retract(X, eta, d) - MR.qf_ld(X, eta, 1.0))[:, :d], cls)
        for c, e in err.items():
            assert e <= 64 * MR.EPS * (1 + [1.0, 1e2, 1e4][c]), (d, r, c, e)


# ---------------------------------------------------------------- the two routes to U V^T, emulated in fp64 NumPy
def gram_route_polar(M, d):
    """What K5 / K12 did before: M (M^T M)^-1/2 through the symmetric eigen-decomposition of the Gram matrix, the
    eigenvalues floored at 1e-28 lambda_max."""
    out = M.copy()
    A = np.swapaxes(M[:, :d, :], 1, 2)
    lam, W = np.linalg.eigh(np.swapaxes(A, 1, 2) @ A)
    lam = np.maximum(lam, np.maximum(1e-28 * lam[:, -1:], 1e-300))
    out[:, :d, :] = np.swapaxes(A @ ((W / np.sqrt(lam)[:, None, :]) @ np.swapaxes(W, 1, 2)), 1, 2)
    return out


def hestenes_route_polar(M, d, tol=2.0 ** -50, sweeps=30):
    """What they do now: one-sided Jacobi on the columns of the (power-of-two scaled) block, U V^T from the normalised
    columns and the accumulated rotations (kernels/manifold.h: jacobi_columns)."""
    out = M.copy()
    for i in range(M.shape[0]):
        a = M[i, :d, :].copy()  # row p = column p of the block
        mx = np.abs(a).max()
        a = np.ldexp(a, -int(np.floor(np.log2(mx)))) if mx > 0 else a
        V = np.eye(d)
        for _ in range(sweeps):
            rotated = False
            for p in range(d):
                for q in range(p + 1, d):
                    al, be, ga = a[p] @ a[p], a[q] @ a[q], a[p] @ a[q]
                    if al > 2.0 ** -600 and be > 2.0 ** -600 and abs(ga) > tol * np.sqrt(al) * np.sqrt(be):
                        rotated = True
                        z = (be - al) / (2 * ga)
                        t = (1.0 if z >= 0 else -1.0) / (abs(z) + np.sqrt(z * z + 1))
                        c = 1 / np.sqrt(t * t + 1)
                        s = t * c
                        a[p], a[q] = c * a[p] - s * a[q], s * a[p] + c * a[q]
                        V[:, p], V[:, q] = c * V[:, p] - s * V[:, q], s * V[:, p] + c * V[:, q]
            if not rotated:
                break
        nrm2 = np.sum(a * a, axis=1)
        inv = np.where(nrm2 > 2.0 ** -600, 1 / np.sqrt(np.where(nrm2 > 0, nrm2, 1)), 0.0)
        out[i, :d, :] = V @ (a * inv[:, None])  # column c = sum_k u_k V[c, k]
    return out


def test_gram_route_loses_what_one_sided_jacobi_keeps(polar_refs):
    """The regression's witness.  At kappa = 1e4 the Gram route is already off the unit sphere by more than 1e-9 (the
    suite's 1e-12 is lost at kappa = 1e2); one-sided Jacobi keeps Y^T Y = I to 1e-14 and the elements within 8 x the
    SVD's own error up to kappa = 1e12."""
    for (d, r), (M, cls, ref) in polar_refs.items():
        gram = gram_route_polar(M, d)
        hest = hestenes_route_polar(M, d)
        k4 = (cls // 3 == 2)
        assert _orth_err(gram[k4][:, :d]) > 1e-9, (d, r)
        assert _orth_err(hest[:, :d]) <= 1e-14, (d, r)
        assert (hest[:, d] == M[:, d]).all()
        svd = np.linalg.svd(np.swapaxes(M[:, :d, :], 1, 2), full_matrices=False)
        Esvd = MR.per_class_max(np.abs(np.swapaxes(svd[0] @ svd[2], 1, 2) - ref[:, :d]), cls)
        Eh = MR.per_class_max(np.abs(hest - ref)[:, :d], cls)
        Eg = MR.per_class_max(np.abs(gram - ref)[:, :d], cls)
        for c in Esvd:
            assert Eh[c] <= 8 * Esvd[c] + 1e-14, (d, r, MR.class_name(c), Eh[c], Esvd[c])
        if r > d:  # (for r = d = 2 the factor is well conditioned and the Gram route's error shows in Y^T Y only)
            assert max(Eg[c] for c in Eg if c // 3 == 3) > 1e-6, (d, r)
