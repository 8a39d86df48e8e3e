"""NumPy restatement of the reference's robust frame alignment, in fp64 and in np.longdouble (the style of
tests/manifold_reference.py, whose rotation_ld is the longdouble projection here):

  singleTranslationAveraging / singleRotationAveraging / singlePoseAveraging   src/DPGO_solver.cpp:23-70
  robustSingleRotationAveraging                                               src/DPGO_solver.cpp:72-135
  robustSinglePoseAveraging                                                   src/DPGO_solver.cpp:137-218
  RobustCost::weight for GNC_TLS, RobustCost::update                          src/DPGO_robust.cpp:80-92, 116-134
  PGOAgent::computeNeighborTransform                                          src/PGOAgent.cpp:515-548
  PGOAgent::computeRobustNeighborTransformTwoStage / ...Transform             src/PGOAgent.cpp:550-602, 604-648
  PGOAgent::initializeInGlobalFrame (the lift)                                src/PGOAgent.cpp:329-337

Rotations are arrays [m, d, d] (R[i][row][col]), translations [m, d]; `dt` is np.float64 or np.longdouble and every
operation runs in it.  The device's tiles [d+1][d] hold the d COLUMNS of the rotation, then the translation: to_tiles /
from_tiles convert.  The seeded input generator of the GPU tests lives here too, so that the CPU test can check what it
promises about every input (planted inlier set recovered; fp64 and longdouble agree in inlier set and iteration count).
"""
import numpy as np

from manifold_reference import LD, rotation_ld

CHI2INV_09_3 = 6.251388631170325  # chi2inv(0.9, 3): RobustCost::computeErrorThresholdAtQuantile(0.9, 3), src/PGOAgent.cpp:630
W_TOL = 1e-8
MU_STEP = 1.4
MU_CAP = 1e-5
TWO_STAGE, POSE = 0, 1
OK, EMPTY, INVALID, FEW_INLIERS = 0, 1, 2, 3
# (inliers, candidates) of the generated groups: one lane / one wave / one stride of 256 lanes on either side
GROUP_SIZES = [(1, 1), (2, 2), (2, 3), (25, 50), (32, 64), (33, 65), (129, 257), (300, 600)]


def angular2chordal(rad):
    """angular2ChordalSO3 (src/DPGO_utils.cpp:514-516)."""
    return 2.0 * np.sqrt(2.0) * np.sin(rad / 2.0)


def mode_defaults(mode):
    """(kappa, tau, barc, max_iterations) of the two modes (src/PGOAgent.cpp:573-580, 628-630; src/DPGO_solver.cpp:104, 181)."""
    if mode == TWO_STAGE:
        return 1.0, 1.0, float(angular2chordal(0.5)), 1000
    return 1.82, 0.01, float(np.sqrt(CHI2INV_09_3)), 10000


def to_tiles(R, t):
    R = np.asarray(R)
    m, d = R.shape[0], R.shape[1]
    tiles = np.zeros((m, d + 1, d), dtype=R.dtype)
    tiles[:, :d, :] = np.swapaxes(R, 1, 2)
    tiles[:, d, :] = t
    return tiles


def from_tiles(tiles):
    tiles = np.asarray(tiles)
    d = tiles.shape[-1]
    return np.swapaxes(tiles[..., :d, :], -1, -2), tiles[..., d, :]


# ---------------------------------------------------------------- projection and single averages
def project_rotation(M, dt):
    """projectToRotationGroup (src/DPGO_utils.cpp:464-478) of one d x d block."""
    if dt is LD:
        return rotation_ld(np.asarray(M, dtype=LD)[None])[0]
    U, _, Vt = np.linalg.svd(np.asarray(M, dtype=np.float64))
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        U = U.copy()
        U[:, -1] = -U[:, -1]
    return U @ Vt


def single_rotation_averaging(R, kappa, dt):
    return project_rotation(np.sum(kappa[:, None, None] * R, axis=0), dt)


def single_translation_averaging(t, tau):
    return np.sum(tau[:, None] * t, axis=0) / np.sum(tau)


def gnc_weight(rSq, mu, barc):
    """RobustCost::weight(sqrt(rSq)) for GNC_TLS (src/DPGO_robust.cpp:80-92), elementwise."""
    r = np.sqrt(rSq)
    rSq = r * r
    bSq = barc * barc
    upper, lower = (mu + 1) / mu * bSq, mu / (mu + 1) * bSq
    with np.errstate(divide="ignore", invalid="ignore"):
        mid = np.sqrt(bSq * mu * (mu + 1) / rSq) - mu
    return np.where(rSq >= upper, rSq.dtype.type(0), np.where(rSq <= lower, rSq.dtype.type(1), mid))


def _robust(R, t, kappa, tau, barc, dt, max_iterations, pose, unit_weights=False):
    """The common body of the two robust averages.  unit_weights: every weight forced to 1 (what a non-robust average
    would return: the tests use it to show that outliers matter)."""
    R = np.asarray(R, dtype=dt)
    t = np.asarray(t, dtype=dt)
    n = R.shape[0]
    kappa = np.asarray(kappa, dtype=dt) * np.ones(n, dtype=dt)
    tau = np.asarray(tau, dtype=dt) * np.ones(n, dtype=dt)
    barc = dt(barc)
    w = np.ones(n, dtype=dt)

    def solve(w):
        Ro = single_rotation_averaging(R, kappa * w, dt)
        to = single_translation_averaging(t, tau * w) if pose else None
        return Ro, to

    def residuals(Ro, to):
        rSq = kappa * np.sum((Ro[None] - R) ** 2, axis=(1, 2))
        if pose:
            rSq = rSq + tau * np.sum((to[None] - t) ** 2, axis=1)
        return rSq

    Ro, to = solve(w)
    rSq = residuals(Ro, to)
    bSq = barc * barc
    with np.errstate(divide="ignore"):
        mu = min(bSq / (2 * np.max(rSq) - bSq), dt(MU_CAP))
    iterations = 0
    if mu > 0 and not unit_weights:
        for _ in range(max_iterations):
            Ro, to = solve(w)
            w = gnc_weight(residuals(Ro, to), mu, barc).astype(dt)
            iterations += 1
            if int(np.sum((w < W_TOL) | (w > 1 - W_TOL))) == n:
                break
            mu = dt(MU_STEP) * mu
    return dict(R=Ro, t=to, weights=w, inliers=np.nonzero(w > 1 - W_TOL)[0], iterations=iterations, mu=mu)


def robust_single_rotation_averaging(R, kappa, barc, dt=np.float64, max_iterations=1000, unit_weights=False):
    """src/DPGO_solver.cpp:72-135."""
    R = np.asarray(R)
    return _robust(R, np.zeros(R.shape[:2]), kappa, 1.0, barc, dt, max_iterations, False, unit_weights)


def robust_single_pose_averaging(R, t, kappa, tau, barc, dt=np.float64, max_iterations=10000, unit_weights=False):
    """src/DPGO_solver.cpp:137-218."""
    return _robust(R, t, kappa, tau, barc, dt, max_iterations, True, unit_weights)


def robust_transform(R, t, mode, dt=np.float64, kappa=None, tau=None, barc=None, min_inliers=2, unit_weights=False):
    """What one group of the device kernel computes: two-stage (src/PGOAgent.cpp:550-602) or pose mode (:604-648) with the
    mode's defaults -> dict(status, R, t, weights, inliers, iterations, mu)."""
    k0, t0, b0, its = mode_defaults(mode)
    kappa = k0 if kappa is None else kappa
    tau = t0 if tau is None else tau
    barc = b0 if barc is None else barc
    R = np.asarray(R)
    if R.shape[0] == 0:
        return dict(status=EMPTY)
    if not (np.isfinite(np.asarray(R, dtype=np.float64)).all() and np.isfinite(np.asarray(t, dtype=np.float64)).all()):
        return dict(status=INVALID)
    if mode == POSE:
        out = robust_single_pose_averaging(R, t, kappa, tau, barc, dt, its, unit_weights)
    else:
        out = robust_single_rotation_averaging(R, kappa, barc, dt, its, unit_weights)
        inl = out["inliers"]
        tt = np.asarray(t, dtype=dt)
        out["t"] = np.sum(tt[inl], axis=0) / dt(len(inl)) if len(inl) else np.zeros(R.shape[1], dtype=dt)
    few = len(out["inliers"]) < min_inliers or (mode == TWO_STAGE and len(out["inliers"]) == 0)
    out["status"] = FEW_INLIERS if few else OK
    return out


# ---------------------------------------------------------------- rigid transforms, candidates, lift
def se_inverse(R, t):
    Rt = np.swapaxes(R, -1, -2)
    return Rt, -np.einsum("...ab,...b->...a", Rt, t)


def se_compose(Ra, ta, Rb, tb):
    return Ra @ Rb, np.einsum("...ab,...b->...a", Ra, tb) + ta


def neighbor_transforms(YLift, X_nbr, T_local, my_pose, slot, incoming, Re, te, dt=np.float64):
    """computeNeighborTransform (src/PGOAgent.cpp:515-548) for m edges.  YLift [r, d]; X_nbr: neighbour tiles [slots, d+1, r];
    T_local: my tiles [n, d+1, d]; Re [m, d, d], te [m, d].  Returns candidate tiles [m, d+1, d]."""
    Y = np.asarray(YLift, dtype=dt)
    X = np.asarray(X_nbr, dtype=dt)[np.asarray(slot)]
    d = Y.shape[1]
    R2 = np.einsum("ka,mck->mac", Y, X[:, :d, :])  # YLift^T X_nbr (:530)
    t2 = np.einsum("ka,mk->ma", Y, X[:, d, :])
    Re, te = np.asarray(Re, dtype=dt), np.asarray(te, dtype=dt)
    Ri, ti = se_inverse(Re, te)
    inc = np.asarray(incoming).astype(bool)
    Rf = np.where(inc[:, None, None], Ri, Re)  # T_frame1_frame2 (:535-543)
    tf = np.where(inc[:, None], ti, te)
    Rl, tl = from_tiles(np.asarray(T_local, dtype=dt)[np.asarray(my_pose)])
    Ra, ta = se_compose(R2, t2, *se_inverse(Rf, tf))  # T_world2_frame1 (:544)
    Rw, tw = se_compose(Ra, ta, *se_inverse(Rl, tl))  # T_world2_world1 (:545)
    return to_tiles(Rw, tw)


def lift_in_frame(YLift, T_world_robot, T_local, dt=np.float64):
    """X_i = YLift (T_world_robot T_local_i) (src/PGOAgent.cpp:329-337): tiles [n, d+1, r]."""
    Y = np.asarray(YLift, dtype=dt)
    Rw, tw = from_tiles(np.asarray(T_world_robot, dtype=dt))
    Rl, tl = from_tiles(np.asarray(T_local, dtype=dt))
    R, t = se_compose(Rw[None], tw[None], Rl, tl)
    n, d = R.shape[0], R.shape[1]
    X = np.zeros((n, d + 1, Y.shape[0]), dtype=dt)
    X[:, :d, :] = np.einsum("ka,nac->nck", Y, R)
    X[:, d, :] = np.einsum("ka,na->nk", Y, t)
    return X


def allowed_error(numpy_error, t_scale=1.0):
    """The tolerance rule of the GPU tests: 32 times the fp64 NumPy restatement's own error against longdouble on the same
    input (the device contracts to fma and sums in another order: a few ulps per operation), not below 1e-14 max(1, |t|)."""
    return max(32.0 * float(numpy_error), 1e-14 * max(1.0, float(t_scale)))


# ---------------------------------------------------------------- seeded inputs
def random_rotations(rng, m, d):
    if d == 2:
        a = rng.uniform(-np.pi, np.pi, m)
        return np.stack([np.stack([np.cos(a), -np.sin(a)], 1), np.stack([np.sin(a), np.cos(a)], 1)], 1)
    q = rng.standard_normal((m, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], 1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)


def small_rotations(rng, m, d, max_angle):
    """Rotations by an angle of at most max_angle about random axes."""
    ang = rng.uniform(-max_angle, max_angle, m)
    if d == 2:
        return np.stack([np.stack([np.cos(ang), -np.sin(ang)], 1), np.stack([np.sin(ang), np.cos(ang)], 1)], 1)
    ax = rng.standard_normal((m, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    K = np.zeros((m, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -ax[:, 2], ax[:, 1], ax[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 0], -ax[:, 1], ax[:, 0]
    return np.eye(3)[None] + np.sin(ang)[:, None, None] * K + (1 - np.cos(ang))[:, None, None] * (K @ K)


def make_group(rng, d, mode, n_in, n_total):
    """One group: truth, n_in inliers (truth times a rotation of at most 0.02 rad, translation noise of norm at most
    0.05), n_total - n_in outliers (uniform rotations, translations within +-100, kept when their residual to the truth in
    the mode's metric exceeds 1.5 barc), shuffled.  Returns (R [n, d, d], t [n, d], planted inlier mask, (Rtrue, ttrue))."""
    kappa, tau, barc, _ = mode_defaults(mode)
    Rtrue = random_rotations(rng, 1, d)[0]
    ttrue = rng.uniform(-10, 10, d)
    Rin = Rtrue[None] @ small_rotations(rng, n_in, d, 0.02)
    tin = ttrue[None] + rng.uniform(-0.05, 0.05, (n_in, d)) / np.sqrt(d)
    Rout, tout = np.zeros((0, d, d)), np.zeros((0, d))
    while len(Rout) < n_total - n_in:
        Rc = random_rotations(rng, 2 * (n_total - n_in) + 8, d)
        tc = rng.uniform(-100, 100, (len(Rc), d))
        rSq = kappa * np.sum((Rc - Rtrue[None]) ** 2, axis=(1, 2))
        if mode == POSE:
            rSq = rSq + tau * np.sum((tc - ttrue[None]) ** 2, axis=1)
        keep = np.sqrt(rSq) > 1.5 * barc
        Rout, tout = np.concatenate([Rout, Rc[keep]]), np.concatenate([tout, tc[keep]])
    Rout, tout = Rout[:n_total - n_in], tout[:n_total - n_in]
    R, t = np.concatenate([Rin, Rout]), np.concatenate([tin, tout])
    mask = np.arange(n_total) < n_in
    perm = rng.permutation(n_total)
    return R[perm], t[perm], mask[perm], (Rtrue, ttrue)


SEED = 20240


def make_case(d, mode, seed=SEED, sizes=GROUP_SIZES):
    """All groups of one (d, mode) launch: dict(R [m, d, d], t [m, d], group_ptr [len(sizes) + 1], planted [m] bool,
    truth [(Rtrue, ttrue)])."""
    rng = np.random.Generator(np.random.PCG64([seed, d, mode]))
    Rs, ts, masks, truth, ptr = [], [], [], [], [0]
    for n_in, n_total in sizes:
        R, t, mask, tr = make_group(rng, d, mode, n_in, n_total)
        Rs.append(R), ts.append(t), masks.append(mask), truth.append(tr)
        ptr.append(ptr[-1] + n_total)
    return dict(R=np.concatenate(Rs), t=np.concatenate(ts), group_ptr=np.array(ptr, dtype=np.int32),
                planted=np.concatenate(masks), truth=truth, d=d, mode=mode)


_CACHE = {}


def reference_runs(d, mode):
    """(case, [fp64 run per group], [longdouble run per group]) of make_case(d, mode): computed once per process."""
    key = (d, mode)
    if key not in _CACHE:
        case = make_case(d, mode)
        gp = case["group_ptr"]
        r64, rld = [], []
        for g in range(len(gp) - 1):
            R, t = case["R"][gp[g]:gp[g + 1]], case["t"][gp[g]:gp[g + 1]]
            r64.append(robust_transform(R, t, mode, np.float64))
            rld.append(robust_transform(R, t, mode, LD))
        _CACHE[key] = (case, r64, rld)
    return _CACHE[key]
