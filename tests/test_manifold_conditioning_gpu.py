"""K5 k_axpby_project (polar projection) and K12 k_round (rounding to SE(d)) on ill-conditioned blocks, class by class
against the longdouble reference of tests/manifold_reference.py; the chordal initialisation on graphs whose relaxed
rotation blocks are nearly singular; the qf retraction at large steps.

Tolerances are set by rule, not in advance: per condition class the device's element error may be 8 x E + 1e-14, E being
the error of the oracle's fp64 LAPACK-SVD restatement against the same reference over the same class (the 8 covers the
device's different summation order and FMA contraction); orthonormality must hold to 1e-14 in EVERY class, because an
SVD-based factor U V^T is orthonormal to round-off whatever kappa is (NumPy's SVD and the NumPy emulation of one-sided
Jacobi in tests/test_manifold_reference_cpu.py both give <= 1.1e-15 on these inputs).  Nothing is compared by a norm
over all poses: one bad class cannot hide behind twenty good ones.

E belongs to a class, not to a launch: it is taken over the 15 or 16 blocks a class has among the NCASE = 333 cases,
and the launches at n = 1 and n = 17 run the first n of those cases against it.  (Among 17 poses a class has one block;
the SVD's error on that one block varies by a factor of 30 from block to block at equal kappa and bounds nothing.)"""
import numpy as np
import pytest

from conftest import matrix_to_tiles, tiles_to_matrix

try:
    import manifold_reference as MR
except AssertionError as e:  # np.longdouble is plain fp64 on this platform
    pytest.skip(str(e), allow_module_level=True)

pytestmark = pytest.mark.gpu

ORTH_TOL = 1e-14
NCASE = max(MR.SIZES)
_cache = {}


def _orth_err(Y):
    """max |Y Y^T - I| per pose of the rotation rows Y [n, d, k]."""
    d = Y.shape[1]
    return np.abs(Y @ np.swapaxes(Y, 1, 2) - np.eye(d)).reshape(len(Y), -1).max(axis=1)


def _polar_case(oracle, d, r):
    """(M, cls, polar_ld(M), E per class) at NCASE poses -- computed once per (d, r) and left unchanged."""
    key = ("polar", d, r)
    if key not in _cache:
        M, cls = MR.polar_cases(d, r, NCASE)
        ref = MR.polar_ld(M)
        E = MR.per_class_max(np.abs(oracle.polar_project(M, d) - ref)[:, :d], cls)
        for a in (M, cls, ref):
            a.setflags(write=False)
        _cache[key] = (M, cls, ref, E)
    return _cache[key]


def _round_case(oracle, d, r):
    """(X, cls, {frame: (anchor tile or None, round_ld, magnitude of the translation terms per pose, E of the rotations
    per class, E of the translations per class)}) at NCASE poses.  Translation errors are taken relative to
    mag_i = |Ya|^T |p_i| + |Ya|^T |pa|, the size of the terms Ya^T p_i - Ya^T pa is summed from: the poses of one class
    span sixteen orders of magnitude, and an absolute error would check the largest of them only."""
    key = ("round", d, r)
    if key not in _cache:
        X, anchor, cls, refl = MR.round_cases(d, r, NCASE)
        frames = {}
        for which, A in (("pose0", None), ("anchor", anchor)):
            ref = MR.round_ld(X, d, A)
            At = X[0] if A is None else A
            mag = (np.abs(X[:, d, :]) @ np.abs(At[:d]).T + np.abs(At[:d]) @ np.abs(At[d])).max(axis=1)
            err = np.abs(oracle.round_trajectory(X, d, A) - ref).astype(np.float64)
            frames[which] = (A, ref, mag, MR.per_class_max(err[:, :d], cls), MR.per_class_max(err[:, d] / mag[:, None], cls))
        X.setflags(write=False)
        _cache[key] = (X, cls, frames)
    return _cache[key]


def _device_project(M, d, r, how):
    """The three ways into K5: LiftedSEManifold::project from host memory, dpgo_manifold_project_device, and
    dpgo_axpby_project_device with three non-zero operands that sum to M exactly (power-of-two splits)."""
    import torch
    import dpgo_amd
    import dpgo_amd.lib as L
    n = M.shape[0]
    if how == "host":
        return matrix_to_tiles(dpgo_amd.LiftedSEManifold(r, d, n).project(tiles_to_matrix(M)), d)
    lib = L.load()
    stream = torch.cuda.current_stream().cuda_stream or None
    out = torch.full((n, d + 1, r), float("nan"), dtype=torch.float64, device="cuda")
    if how == "device":
        Md = torch.tensor(M, dtype=torch.float64, device="cuda")
        L.check(lib.dpgo_manifold_project_device(r, d, n, L.ptr(Md), L.ptr(out), stream))
    else:
        # M = 0.5 * (M / 2) + 2 * (M / 4) + (-0.25) * (-M): every product and both sums are exact in fp64
        A, B, Cm = (torch.tensor(v, dtype=torch.float64, device="cuda") for v in (M / 2, M / 4, -M))
        L.check(lib.dpgo_axpby_project_device(r, d, n, 0.5, L.ptr(A), 2.0, L.ptr(B), -0.25, L.ptr(Cm), 1, L.ptr(out),
                                              stream))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_polar_classes(out, M, cls, ref, E, d, label):
    """Per class: orthonormal to ORTH_TOL, elements within 8 E + 1e-14; the translation row bitwise the input."""
    assert np.isfinite(out).all(), label
    assert (out[:, d] == M[:, d]).all(), label
    orth = MR.per_class_max(_orth_err(out[:, :d]), cls)
    err = MR.per_class_max(np.abs(out - ref)[:, :d], cls)
    bad = []
    for c in sorted(err):
        print("%s %-24s E %.2e  device err %.2e  orth %.2e" % (label, MR.class_name(c), E[c], err[c], orth[c]))
        if not orth[c] <= ORTH_TOL:
            bad.append((MR.class_name(c), "orth", orth[c]))
        if not err[c] <= 8 * E[c] + 1e-14:
            bad.append((MR.class_name(c), "err", err[c], "E", E[c]))
    assert not bad, (label, bad)


@pytest.mark.parametrize("d,r", MR.DR)
def test_polar_projection_per_condition_class(oracle, d, r):
    """K5 at every (d, r), n = 1, 17 and 333 (one lane group; less than a wavefront; two workgroups, the last ragged),
    through the host entry, the device entry and the fused a A + b B + c C entry: kappa from 1 to 1e12, geometric and
    clustered spectra, overall scales 1e-8 .. 1e8, each class on its own."""
    Mall, call, refall, E = _polar_case(oracle, d, r)
    for n in MR.SIZES:
        M, cls, ref = Mall[:n], call[:n], refall[:n]
        for how in ("host", "device", "axpby"):
            _check_polar_classes(_device_project(M, d, r, how), M, cls, ref, E, d, "polar d=%d r=%d n=%d %s" % (d, r, n, how))


@pytest.mark.parametrize("d,r", MR.DR)
def test_rounding_per_condition_class(oracle, d, r):
    """K12 at every (d, r), n = 1, 17 and 333, host and device entries, in the frame of pose 0 and of an explicit
    anchor: X_i = (Ylift B_i)^T with B_i the case blocks, a quarter of them reflected (det < 0, geometric spectra).  Per
    class det = +1 to 1e-13, orthonormal to 1e-14, rotation elements within 8 E + 1e-14 and translations within 8 E of
    theirs (relative to the size of their terms, see _round_case), E = the error of oracle.round_trajectory against
    round_ld over the class."""
    import torch
    import dpgo_amd
    Xall, call, frames = _round_case(oracle, d, r)
    for n in MR.SIZES:
        X, cls = Xall[:n], call[:n]
        for which, (A, refall, magall, Er, Et) in frames.items():
            ref, mag = refall[:n], magall[:n]
            at = None if A is None else A.T
            Tm = dpgo_amd.round_trajectory(tiles_to_matrix(X), r, d, at)
            got_h = np.ascontiguousarray(np.asfortranarray(Tm).T).reshape(n, d + 1, d)
            got_d = dpgo_amd.round_trajectory_device(torch.tensor(X, dtype=torch.float64, device="cuda"), at).cpu().numpy()
            for entry, got in (("host", got_h), ("device", got_d)):
                label = "round d=%d r=%d n=%d %s %s" % (d, r, n, which, entry)
                assert np.isfinite(got).all(), label
                det = MR.per_class_max(np.abs(np.linalg.det(got[:, :d]) - 1), cls)
                orth = MR.per_class_max(_orth_err(got[:, :d]), cls)
                err = MR.per_class_max(np.abs(got - ref)[:, :d], cls)
                terr = MR.per_class_max(np.abs(got - ref)[:, d] / mag[:, None], cls)
                bad = []
                for c in sorted(err):
                    print("%s %-24s E %.2e  device err %.2e  orth %.2e  |det-1| %.2e  Et %.2e  device terr %.2e" % (
                        label, MR.class_name(c), Er[c], err[c], orth[c], det[c], Et[c], terr[c]))
                    if not det[c] <= 1e-13:
                        bad.append((MR.class_name(c), "det", det[c]))
                    if not orth[c] <= ORTH_TOL:
                        bad.append((MR.class_name(c), "orth", orth[c]))
                    if not err[c] <= 8 * Er[c] + 1e-14:
                        bad.append((MR.class_name(c), "err", err[c], "E", Er[c]))
                    if not terr[c] <= 8 * Et[c]:
                        bad.append((MR.class_name(c), "terr", terr[c], "E", Et[c]))
                assert not bad, (label, bad)


@pytest.mark.parametrize("d,r", [(2, 2), (2, 3), (3, 3), (3, 5), (3, 6)])
def test_rank_deficient_blocks_stay_bounded(oracle, d, r):
    """Blocks the polar factor is not defined for -- zero, rank 1, two parallel columns -- and blocks beyond what fp64
    resolves (kappa = 1e14, 1e16, 1e20), between full-rank case blocks.  `isfinite` alone admits outputs of size 1e11;
    what the projection owes is an output no longer than a partial isometry: every singular value <= 1 + 1e-12.  Blocks
    of kappa <= 1e12 next to them stay orthonormal to 1e-14 and within their class tolerance."""
    n = 63
    Mall, call, refall, E = _polar_case(oracle, d, r)
    M, cls = Mall[:n].copy(), call[:n]
    rng = np.random.default_rng(31 * d + r)
    special = {}
    for k, i in enumerate(range(2, n, 5)):
        kind = ["zero", "rank1", "parallel", 1e14, 1e16, 1e20][k % 6]
        sc = MR.SCALES[k % 3]
        if kind == "zero":
            M[i, :d] = 0.0
        elif kind == "rank1":
            M[i, :d] = sc * np.outer(rng.standard_normal(d), rng.standard_normal(r))
        elif kind == "parallel":
            M[i, :d] = sc * rng.standard_normal((d, r))
            M[i, d - 1] = -2.0 * M[i, 0]
        else:
            s = kind ** (-np.arange(d) / (d - 1.0))
            M[i, :d] = sc * ((MR._orthonormal(rng, r, d) * s) @ MR._orthonormal(rng, d, d).T).T
        special[i] = kind
    good = np.setdiff1d(np.arange(n), list(special))
    ref = refall[:n][good]
    for how in ("host", "device", "axpby"):
        out = _device_project(M, d, r, how)
        assert np.isfinite(out).all(), how
        assert (out[:, d] == M[:, d]).all(), how
        smax = np.linalg.svd(out[:, :d], compute_uv=False).max(axis=1)
        print("rank-deficient d=%d r=%d %s: largest singular value of an output block %.16g; by kind %s" % (
            d, r, how, smax.max(), {str(special[i]): float(smax[i]) for i in special}))
        assert (smax <= 1 + 1e-12).all(), (how, {i: (special.get(i), smax[i]) for i in np.nonzero(smax > 1 + 1e-12)[0]})
        assert (out[[i for i in special if special[i] == "zero"], :d] == 0).all()
        _check_polar_classes(out[good], M[good], cls[good], ref, E, d, "neighbours d=%d r=%d %s" % (d, r, how))


def _conflict_chain(d, n=40, seed=0):
    """A chain 0 -> 1 -> ... -> n-1 of exact relative poses in which five poses j hang on j-1 by a PAIR of edges whose
    measured rotations differ by a half turn (about the first axis for d = 3; -I for d = 2), with kappa in the ratio
    1 : 1 + eps, eps in {1e-2, 1e-5, 1e-8}; the chain itself steps over such a pose (j-1 -> j+1).  The relaxed rotation
    block of pose j is the kappa-weighted mean of two rotations half a turn apart: singular values (1, eps/2, eps/2)
    for d = 3 and (eps/2, eps/2) for d = 2, with the larger kappa deciding which rotation is nearest.
    Returns (arrays for either Measurements class, the conflicted poses)."""
    rng = np.random.default_rng(7 + d + seed)

    def rot():
        Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        if np.linalg.det(Q) < 0:
            Q[:, 0] = -Q[:, 0]
        return Q
    Rg = np.stack([rot() for _ in range(n)])
    tg = 3.0 * rng.standard_normal((n, d))
    half = -np.eye(d)
    half[0, 0] = 1.0 if d == 3 else -1.0
    conflicted = {5: 1e-2, 13: 1e-5, 21: 1e-8, 29: 1e-8, 36: 1e-5}
    p1, p2, R, t, kappa = [], [], [], [], []

    def edge(i, j, Rij=None, k=1.0):
        p1.append(i)
        p2.append(j)
        R.append(Rg[i].T @ Rg[j] if Rij is None else Rij)
        t.append(Rg[i].T @ (tg[j] - tg[i]))
        kappa.append(k)
    for j in range(1, n):
        if j in conflicted:
            edge(j - 1, j, k=1.0)
            edge(j - 1, j, Rij=Rg[j - 1].T @ Rg[j] @ half, k=1.0 + conflicted[j])
        elif j - 1 in conflicted:
            edge(j - 2, j)
        else:
            edge(j - 1, j)
    m = len(p1)
    z = np.zeros(m, dtype=np.int64)
    arrays = (d, z, np.array(p1, dtype=np.int64), z.copy(), np.array(p2, dtype=np.int64), np.array(R), np.array(t),
              np.array(kappa), np.ones(m), np.ones(m), np.zeros(m, dtype=bool))
    return arrays, sorted(conflicted)


@pytest.mark.parametrize("d", [2, 3])
def test_chordal_initialisation_returns_rotations(oracle, d):
    """dpgo_chordal_initialization on graphs whose relaxed blocks are nearly singular (conflicting measurements, as
    outliers produce): every rotation block of the initial guess is a rotation -- |det - 1| <= 1e-12, orthonormal to
    1e-13 -- and the translations are the least-squares translations FOR THOSE rotations (the oracle's
    recoverTranslations on the device's rotations) to the tolerance of the device's PCG.  The rotations themselves are
    not compared with the oracle's: a relaxed block is known only to the solve's tolerance times kappa.

    Translation bound: PCG stops at |r| <= tol |b| (tol = 1e-13, x0 = 0), so |x - x*| <= cond(A) tol |x*| in the 2-norm,
    A the reduced translation Laplacian; the recurrence's residual drifts from the true one by O(eps cond(A)) per
    iteration and the oracle's sparse LU adds as much: 64 eps cond(A) |x*| are allowed for both."""
    import dpgo_amd
    from dpgo_amd.initialization import chordal_initialization
    n = 40
    arrays, conflicted = _conflict_chain(d, n)
    om = oracle.Measurements(*arrays)
    pm = dpgo_amd.RelativeSEMeasurements(*[np.copy(a) if isinstance(a, np.ndarray) else a for a in arrays])
    T, its = chordal_initialization(pm, n, return_iterations=True)
    assert T.shape == (n, d + 1, d) and np.isfinite(T).all() and min(its) >= 1
    Rt = T[:, :d, :]  # rows = columns of R_i
    det, orth = np.abs(np.linalg.det(Rt) - 1), _orth_err(Rt)
    print("chordal d=%d: max |det-1| %.2e, max orth %.2e; at the conflicted poses %s: |det-1| %s orth %s" % (
        d, det.max(), orth.max(), conflicted, det[conflicted], orth[conflicted]))
    assert det.max() <= 1e-12, (np.argmax(det), det.max())
    assert orth.max() <= 1e-13, (np.argmax(orth), orth.max())
    t_ref = oracle.recover_translations(om, n, np.swapaxes(Rt, 1, 2))
    Lap = np.zeros((n, n))
    for i, j, tau in zip(om.p1, om.p2, om.tau):
        Lap[i, i] += tau
        Lap[j, j] += tau
        Lap[i, j] -= tau
        Lap[j, i] -= tau
    cond = np.linalg.cond(Lap[1:, 1:])
    bound = (1e-13 + 64 * MR.EPS) * cond * np.linalg.norm(t_ref)
    terr = np.linalg.norm(T[:, d, :] - t_ref)
    print("chordal d=%d: |t - t_ref| %.2e, bound %.2e (cond %.1f, |t_ref| %.2e)" % (d, terr, bound, cond, np.linalg.norm(t_ref)))
    assert terr <= bound, (terr, bound)


@pytest.mark.parametrize("d,r", MR.DR)
def test_retraction_at_large_steps(oracle, d, r):
    """K4 k_retract with |eta_i| = 1, 1e2 and 1e4 (the default initial trust-region radius is 100) against the
    Householder QR of the longdouble reference: the oracle's qf_retract is the same modified Gram-Schmidt as qf_col, so
    the existing comparison is not independent.  Per step-size class the device stays within 8 x the oracle's error
    + 1e-15."""
    import dpgo_amd
    n = 333
    X, eta, cls = MR.retraction_cases(d, r, n)
    ref = MR.qf_ld(X, eta, 1.0)
    E = MR.per_class_max(np.abs(oracle.qf_retract(X, eta, d) - ref), cls)
    out = matrix_to_tiles(dpgo_amd.LiftedSEManifold(r, d, n).Retraction(tiles_to_matrix(X), tiles_to_matrix(eta)), d)
    err = MR.per_class_max(np.abs(out - ref), cls)
    for c in sorted(E):
        print("retract d=%d r=%d |eta| %.0e: E %.2e  device err %.2e" % (d, r, [1, 1e2, 1e4][c], E[c], err[c]))
    for c in sorted(E):
        assert err[c] <= 8 * E[c] + 1e-15, (d, r, c, err[c], E[c])
