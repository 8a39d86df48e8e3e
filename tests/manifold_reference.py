"""np.longdouble restatement of the per-pose dense numerics of kernels/manifold.h -- the polar projection (K5
k_axpby_project), the rounding to SE(d) (K12 k_round) and the qf retraction (K4 k_retract) -- with seeded generators of
ill-conditioned case blocks, used by tests/test_manifold_reference_cpu.py and tests/test_manifold_conditioning_gpu.py.
Nothing here calls the oracle's fp64 code, and nothing here takes a singular value decomposition: the orthogonal factor
comes from a Householder QR followed by a scaled Newton iteration (Higham, Functions of Matrices, Alg. 8.20), so it is
independent of both the oracle's LAPACK SVD and the device's one-sided Jacobi.

Layouts: tiles [n, d+1, r] (the tile view of the r x (d+1)n matrix: X[i, :d, :] = Y_i^T, X[i, d, :] = p_i); rounded
tiles [n, d+1, d] (rows 0..d-1 = the columns of the rotation, row d = the translation).

Conditioning (why the tolerances of the tests are measured, not constants): the orthogonal polar factor of an r x d
block with singular values s_1 >= ... >= s_d moves by |dM| / s_d when r > d and by 2 |dM| / (s_{d-1} + s_d) when r = d
(Higham, Thm 8.9/8.10); the nearest ROTATION of a block with det < 0 by |dM| / (s_{d-1} - s_d), which is why reflected
case blocks use geometric spectra only: with s_{d-1} = s_d the nearest rotation is not unique and no reference exists.
This module's own error is therefore 2^-64 kappa, a factor 2^-11 below anything fp64 can reach.

Case classes: class = 3 * (index of kappa in KAPPAS) + (index of the spectrum in SPECTRA); 21 classes, interleaved along
the pose index as class(i) = (i + 4 (i // 21)) % 21: every round of 21 poses holds each class once, shifted by four
places from round to round, so that one class meets at least 14 of the 16 lane groups of a wavefront for d = 3 and 15 of
the 21 for d = 2 (the shift of four is the one that spreads both best), with the overall scale cycling through SCALES
once per round.  n = 333 gives 15 or 16 blocks per class and a ragged last workgroup.  Every generator draws pose by
pose from one seeded stream, so the cases of a smaller n are the first n poses of a larger one: the tests run n = 1 and
n = 17 as prefixes of the n = 333 cases and hold them to the E of the WHOLE class (a class has one block among the
first 17, and the error of one SVD is no bound for another).

Measured E, the largest element error of the oracle's fp64 SVD restatement against this module per kappa class (max
over every (d, r), spectrum and scale at n = 333, as printed by tests/test_manifold_conditioning_gpu.py; the device is held
to 8 E + 1e-14 of ITS class, (d, r) and spectrum, which the tests compute themselves -- these are for orientation):
    kappa   polar     rounding
    1e+00   7.2e-16   5.0e-15
    1e+02   2.2e-14   9.9e-15
    1e+04   1.9e-12   6.3e-13
    1e+06   1.4e-10   7.6e-11
    1e+08   1.2e-08   5.4e-09
    1e+10   2.3e-06   7.7e-07
    1e+12   1.4e-04   7.4e-05
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "np.longdouble is not an 80-bit (or wider) format here"

EPS = float(np.finfo(np.float64).eps)
DR = [(2, 2), (2, 3), (2, 4), (2, 5), (3, 3), (3, 4), (3, 5), (3, 6)]  # DPGO_FOR_DR (csrc/host.h)
KAPPAS = [1.0, 1e2, 1e4, 1e6, 1e8, 1e10, 1e12]
SPECTRA = ["geometric", "one_small", "one_large"]  # s geometric 1 .. 1/kappa; (1,..,1,1/kappa); (1,1/kappa,..,1/kappa)
SCALES = [1e-8, 1.0, 1e8]
NCLASS = len(KAPPAS) * len(SPECTRA)
SIZES = [1, 17, 333]

def class_kappa(cls):
    return np.asarray(KAPPAS)[np.asarray(cls) // len(SPECTRA)]


def class_name(c):
    return "kappa=%.0e/%s" % (KAPPAS[c // len(SPECTRA)], SPECTRA[c % len(SPECTRA)])


def _ld(a):
    return np.array(a, dtype=LD)


# ---------------------------------------------------------------- small dense building blocks (batched, longdouble)
def _householder_qr(A):
    """Thin QR of a batch A [n, m, k] (m >= k) by Householder reflections: (Q [n, m, k], R [n, k, k]), diag(R) of
    either sign.  A zero column leaves its reflector out (Q stays orthonormal)."""
    A = _ld(A)
    n, m, k = A.shape
    R = A.copy()
    vs = []
    for j in range(k):
        x = R[:, j:, j].copy()
        nx = np.sqrt(np.sum(x * x, axis=1))
        alpha = np.where(x[:, 0] >= 0, -nx, nx)
        v = x
        v[:, 0] -= alpha
        nv = np.sqrt(np.sum(v * v, axis=1))
        v = v / np.where(nv > 0, nv, LD(1))[:, None]
        v[nv == 0] = 0
        R[:, j:, :] -= 2 * v[:, :, None] * np.einsum("ni,nij->nj", v, R[:, j:, :])[:, None, :]
        vs.append(v)
    Q = np.zeros((n, m, k), dtype=LD)
    Q[:, np.arange(k), np.arange(k)] = 1
    for j in reversed(range(k)):
        v = vs[j]
        Q[:, j:, :] -= 2 * v[:, :, None] * np.einsum("ni,nij->nj", v, Q[:, j:, :])[:, None, :]
    return Q, np.triu(R[:, :k, :])


def _inv(A):
    """Batched inverse [n, d, d] by Gauss-Jordan with partial pivoting (an adjugate would lose the small minors)."""
    A = _ld(A)
    n, d, _ = A.shape
    W = np.concatenate([A, np.broadcast_to(np.eye(d, dtype=LD), (n, d, d))], axis=2).copy()
    idx = np.arange(n)
    for k in range(d):
        p = k + np.argmax(np.abs(W[:, k:, k]), axis=1)
        rk, rp = W[idx, k].copy(), W[idx, p].copy()
        W[idx, k], W[idx, p] = rp, rk
        W[:, k] = W[:, k] / W[:, k, k:k + 1].copy()
        for j in range(d):
            if j != k:
                W[:, j] = W[:, j] - W[:, j, k:k + 1].copy() * W[:, k]
    return W[:, :, d:]


def _det(A):
    d = A.shape[-1]
    if d == 2:
        return A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
    return (A[:, 0, 0] * (A[:, 1, 1] * A[:, 2, 2] - A[:, 1, 2] * A[:, 2, 1])
            - A[:, 0, 1] * (A[:, 1, 0] * A[:, 2, 2] - A[:, 1, 2] * A[:, 2, 0])
            + A[:, 0, 2] * (A[:, 1, 0] * A[:, 2, 1] - A[:, 1, 1] * A[:, 2, 0]))


def _norm1(A):
    return np.max(np.sum(np.abs(A), axis=1), axis=1)


def _norminf(A):
    return np.max(np.sum(np.abs(A), axis=2), axis=1)


def _newton_polar(A, max_iter=100):
    """Orthogonal polar factor of a batch of nonsingular square blocks: X <- (g X + X^-T / g) / 2 with Higham's
    (1, inf)-norm scaling g until the step is small, then unscaled to convergence."""
    X = _ld(A)
    X = X / np.max(np.abs(X), axis=(1, 2))[:, None, None]
    unscaled = np.zeros(len(X), dtype=bool)
    for _ in range(max_iter):
        Xi = _inv(X)
        g = ((_norm1(Xi) * _norminf(Xi)) / (_norm1(X) * _norminf(X))) ** LD(0.25)
        g = np.where(unscaled, LD(1), g)[:, None, None]
        Xn = (g * X + np.swapaxes(Xi, 1, 2) / g) / 2
        step = np.max(np.abs(Xn - X), axis=(1, 2))
        X = Xn
        if (unscaled & (step <= 8 * np.finfo(LD).eps)).all():
            break
        unscaled |= step < 1e-2
    else:
        raise RuntimeError("Newton polar iteration did not converge")
    return X


def _sym_eig_smallest(H):
    """Unit eigenvector of the smallest eigenvalue of ONE symmetric d x d block (cyclic two-sided Jacobi, longdouble)."""
    H = _ld(H)
    d = H.shape[0]
    W = np.eye(d, dtype=LD)
    for _ in range(60):
        off = sum(H[p, q] ** 2 for p in range(d) for q in range(p + 1, d))
        if off <= (np.finfo(LD).eps ** 2) * np.sum(np.diag(H) ** 2) * LD(1e-6):
            break
        for p in range(d):
            for q in range(p + 1, d):
                if H[p, q] == 0:
                    continue
                th = (H[q, q] - H[p, p]) / (2 * H[p, q])
                t = (1 if th >= 0 else -1) / (abs(th) + np.sqrt(th * th + 1))
                c = 1 / np.sqrt(t * t + 1)
                s = t * c
                J = np.eye(d, dtype=LD)
                J[p, p] = J[q, q] = c
                J[p, q], J[q, p] = s, -s
                H = J.T @ H @ J
                W = W @ J
    v = W[:, int(np.argmin(np.diag(H)))]
    return v / np.sqrt(np.sum(v * v))


# ---------------------------------------------------------------- the references
def polar_ld(M):
    """LiftedSEManifold::project in longdouble.  M: tiles [n, d+1, r] (fp64 or longdouble); per pose a Householder thin
    QR of the r x d block A = Q R, then the Newton polar factor W of R: U V^T = Q W.  The translation row is copied.
    Blocks must have full column rank."""
    M = _ld(M)
    d = M.shape[1] - 1
    out = M.copy()
    Q, R = _householder_qr(np.swapaxes(M[:, :d, :], 1, 2))
    out[:, :d, :] = np.swapaxes(Q @ _newton_polar(R), 1, 2)
    return out


def rotation_ld(M):
    """projectToRotationGroup (src/DPGO_utils.cpp:464-478) of a batch of d x d blocks [n, d, d] in longdouble: the polar
    factor W of M = W H; det W = det U det V of any SVD M = U S V^T.  Where it is negative the result is
    U diag(1, .., 1, -1) V^T = W (I - 2 v v^T) with v the eigenvector of H = W^T M for its smallest eigenvalue (the
    direction of the smallest singular value).  That direction is unique only when s_{d-1} > s_d."""
    M = _ld(M)
    W = _newton_polar(M)
    neg = np.nonzero(_det(W) < 0)[0]
    for i in neg:
        H = W[i].T @ M[i]
        v = _sym_eig_smallest((H + H.T) / 2)
        W[i] = W[i] - 2 * np.outer(W[i] @ v, v)
    return W


def round_ld(X, d, anchor=None):
    """PGOAgent::getTrajectoryInLocalFrame (anchor None: pose 0) / InGlobalFrame (src/PGOAgent.cpp:718-767) in
    longdouble from the fp64 inputs as given: T_i = [rotation_ld(Ya^T Y_i) | Ya^T p_i - Ya^T pa].  X: tiles [n, d+1, r];
    anchor: one tile [d+1, r].  Returns tiles [n, d+1, d]."""
    X = _ld(X)
    A = X[0] if anchor is None else _ld(anchor)
    Ya = A[:d]  # [d, r] = Ya^T
    n = X.shape[0]
    Mb = np.einsum("ak,nbk->nab", Ya, X[:, :d, :])  # M_i[a, b] = sum_k Ya[k, a] Y_i[k, b]
    T = np.zeros((n, d + 1, d), dtype=LD)
    T[:, :d, :] = np.swapaxes(rotation_ld(Mb), 1, 2)
    T[:, d, :] = X[:, d, :] @ Ya.T - Ya @ A[d]
    return T


def qf_ld(X, eta, scale):
    """ROPTLIB Stiefel::qfRetraction of scale * eta at X in longdouble: the Q factor of a Householder thin QR of
    Y + scale eta with the diagonal of R made positive; Euclidean factor p + scale eta.  Tiles [n, d+1, r]."""
    X, eta = _ld(X), _ld(eta)
    d = X.shape[1] - 1
    out = X + LD(scale) * eta
    Q, R = _householder_qr(np.swapaxes(out[:, :d, :], 1, 2))
    sg = np.where(np.diagonal(R, axis1=1, axis2=2) < 0, LD(-1), LD(1))
    out[:, :d, :] = np.swapaxes(Q * sg[:, None, :], 1, 2)
    return out


# ---------------------------------------------------------------- case generators
def _spectrum(kind, kappa, d):
    if kind == "geometric":
        return kappa ** (-np.arange(d) / (d - 1.0))
    s = np.ones(d)
    if kind == "one_small":
        s[-1] = 1.0 / kappa
    else:
        s[1:] = 1.0 / kappa
    return s


def pose_classes(n):
    """(class, index into SCALES) of poses 0 .. n-1."""
    i = np.arange(n)
    return (i + 4 * (i // NCLASS)) % NCLASS, (i // NCLASS) % len(SCALES)


def _orthonormal(rng, m, k):
    Q, _ = np.linalg.qr(rng.standard_normal((m, k)))
    return Q


def polar_cases(d, r, n, seed=0):
    """Tiles M [n, d+1, r] whose r x d blocks are scale * U diag(s) V^T (U r x d orthonormal, V orthogonal, s by the
    pose's class) with random translations of the same scale.  Returns (M, cls [n])."""
    rng = np.random.default_rng(1000 * seed + 10 * d + r)
    cls, sci = pose_classes(n)
    M = np.zeros((n, d + 1, r))
    for i in range(n):
        s = _spectrum(SPECTRA[cls[i] % len(SPECTRA)], KAPPAS[cls[i] // len(SPECTRA)], d)
        B = (_orthonormal(rng, r, d) * s) @ _orthonormal(rng, d, d).T
        sc = SCALES[sci[i]]
        M[i, :d] = sc * B.T
        M[i, d] = sc * rng.standard_normal(r)
    return M, cls


def round_cases(d, r, n, seed=0):
    """A lifted trajectory for the rounding: X_i = (Ylift B_i)^T with B_i = scale * U diag(s) V^T the d x d case blocks,
    det B_i > 0 except on the reflected poses (det < 0: the branch of projectToRotationGroup that negates the direction
    of the smallest singular value).  Reflected poses are taken from the GEOMETRIC spectra with kappa > 1 only -- three
    in four of them, a quarter of all poses: with s_{d-1} = s_d (both clustered spectra for d = 2, one_large for d = 3,
    and kappa = 1) the nearest rotation of a reflected block is not unique, so there is nothing to compare with.
    Pose 0 is of class 0 (kappa = 1), so it serves as the anchor of the local frame; `anchor` is a separate
    well-conditioned tile for the global frame.  Returns (X [n, d+1, r], anchor [d+1, r], cls [n], reflected [n])."""
    rng = np.random.default_rng(2000 * seed + 10 * d + r)
    cls, sci = pose_classes(n)
    Ylift = _orthonormal(rng, r, d)
    Qa = _orthonormal(rng, d, d)
    if np.linalg.det(Qa) < 0:  # a rotation, as B_0 is: the sign of det(Ya^T Y_i) is that of det B_i in either frame
        Qa[:, 0] = -Qa[:, 0]
    anchor = np.zeros((d + 1, r))
    anchor[:d] = (Ylift @ Qa).T + 1e-3 * rng.standard_normal((d, r))
    anchor[d] = rng.standard_normal(r)
    X = np.zeros((n, d + 1, r))
    reflected = np.zeros(n, dtype=bool)
    for i in range(n):
        kind, kappa = SPECTRA[cls[i] % len(SPECTRA)], KAPPAS[cls[i] // len(SPECTRA)]
        U, V = _orthonormal(rng, d, d), _orthonormal(rng, d, d)
        reflected[i] = kind == "geometric" and kappa > 1 and (i // NCLASS) % 4 != 3
        if (np.linalg.det(U) * np.linalg.det(V) < 0) != reflected[i]:
            U[:, 0] = -U[:, 0]
        sc = SCALES[sci[i]]
        X[i, :d] = sc * (Ylift @ ((U * _spectrum(kind, kappa, d)) @ V.T)).T
        X[i, d] = sc * rng.standard_normal(r)
    return X, anchor, cls, reflected


def retraction_cases(d, r, n, seed=0):
    """(X, eta): a point of the manifold (fp64 polar factors of random blocks, orthonormal to round-off) and tangent-ish
    steps whose norm per pose cycles through 1, 1e2 and 1e4 (the default initial trust-region radius is 100).  Returns
    (X, eta, cls [n]) with cls the index of the step norm."""
    rng = np.random.default_rng(3000 * seed + 10 * d + r)
    X = np.zeros((n, d + 1, r))
    for i in range(n):
        X[i, :d] = _orthonormal(rng, r, d).T
    X[:, d] = rng.standard_normal((n, r))
    eta = rng.standard_normal((n, d + 1, r))
    cls = np.arange(n) % 3
    eta *= (np.array([1.0, 1e2, 1e4])[cls] / np.sqrt(np.sum(eta * eta, axis=(1, 2))))[:, None, None]
    return X, eta, cls


def per_class_max(err, cls):
    """max of err [n, ...] over the poses of each class: {class: float}."""
    err = np.asarray(err, dtype=np.float64).reshape(len(cls), -1).max(axis=1)
    return {int(c): float(err[cls == c].max()) for c in np.unique(cls)}
