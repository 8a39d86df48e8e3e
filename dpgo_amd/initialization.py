"""Initial guesses, through the C ABI -- no SciPy, no CPU solver in the product path.

  chordal_initialization    reference src/DPGO_solver.cpp:220-269 (+ constructBMatrices / recoverTranslations,
                            src/DPGO_utils.cpp:346-462)  ->  dpgo_chordal_initialization: the two least-squares problems
                            are solved on the device (Jacobi-preconditioned CG over the block-SpMM of the hot path,
                            SO(d) projection by the rounding kernel)
  odometry_initialization   reference src/DPGO_solver.cpp:271-303  ->  dpgo_odometry_initialization (a sequential
                            composition along the chain: host code inside the library)
  robustSingleRotationAveraging / robustSinglePoseAveraging
                            reference src/DPGO_solver.cpp:72-135, 137-218  ->  dpgo_robust_average (k_robust_average: the
                            whole GNC-TLS loop in one kernel; what a waiting agent averages its candidate frame
                            transforms with)

Results are tiles T[n, d+1, d] (tile i = [R_i^T ; t_i], i.e. the d x (d+1) pose in the reference's column-major layout).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as L
from .measurements import RelativeSEMeasurements


def _arrays(meas: RelativeSEMeasurements):
    return (L.i32(meas.p1), L.i32(meas.p2), L.f64(meas.R), L.f64(meas.t), L.f64(meas.kappa), L.f64(meas.tau))


def chordal_initialization(meas: RelativeSEMeasurements, num_poses: int, tol: float = 0.0, max_iter: int = 0,
                           device: int = 0, return_iterations: bool = False):
    """chordalInitialization for the poses of ONE robot (frames 0 .. n-1); pose 0 is the identity."""
    d, n = meas.d, int(num_poses)
    p1, p2, R, t, kappa, tau = _arrays(meas)
    T = np.zeros((n, d + 1, d))
    its = (C.c_int * 2)()
    L.check(L.load().dpgo_chordal_initialization(d, n, len(meas), L.ptr(p1), L.ptr(p2), L.ptr(R), L.ptr(t), L.ptr(kappa),
                                                 L.ptr(tau), float(tol), int(max_iter), L.ptr(T), its, int(device)))
    return (T, (its[0], its[1])) if return_iterations else T


def angular2ChordalSO3(rad: float) -> float:
    """angular2ChordalSO3 (src/DPGO_utils.cpp:514-516): chordal distance of two rotations `rad` apart."""
    return 2.0 * np.sqrt(2.0) * np.sin(rad / 2.0)


def average_params(two_stage: bool = True, barc: float = None, min_inliers: int = 2, max_iterations: int = 0):
    """dpgo_average_params with the reference's values for the mode (dpgo_average_params_default)."""
    p = L.AverageParamsC()
    L.load().dpgo_average_params_default(L.AVERAGE_TWO_STAGE if two_stage else L.AVERAGE_POSE, C.byref(p))
    if barc is not None:
        p.barc = float(barc)
    p.min_inliers, p.max_iterations = int(min_inliers), int(max_iterations)
    return p


def candidate_tiles(RVec, tVec=None) -> np.ndarray:
    """Rotations R_i (d x d) and translations t_i -> candidate tiles [m, d+1, d] (the d columns of R_i, then t_i)."""
    Rs = np.asarray(RVec, dtype=np.float64)
    m, d = Rs.shape[0], Rs.shape[1]
    tiles = np.zeros((m, d + 1, d))
    tiles[:, :d, :] = np.swapaxes(Rs, 1, 2)
    if tVec is not None:
        tiles[:, d, :] = np.asarray(tVec, dtype=np.float64).reshape(m, d)
    return tiles


def robust_average(tiles: np.ndarray, params, kappa=None, tau=None, group_ptr=None, device: int = 0):
    """dpgo_robust_average on host arrays: candidate tiles [m, d+1, d] in groups (default: one group) ->
    (records [ngroups] of lib.AverageResultC, weights [m])."""
    tiles = L.f64(tiles)
    m, d = tiles.shape[0], tiles.shape[2]
    gp = L.i32([0, m] if group_ptr is None else group_ptr)
    ng = len(gp) - 1
    k = None if kappa is None else L.f64(kappa)
    t = None if tau is None else L.f64(tau)
    if (k is not None and k.shape != (m,)) or (t is not None and t.shape != (m,)):
        raise ValueError("kappa / tau need one entry per candidate")
    w = np.zeros(max(m, 1))
    res = (L.AverageResultC * ng)()
    L.check(L.load().dpgo_robust_average(d, ng, L.ptr(gp), L.ptr(tiles), L.ptr(k), L.ptr(t), C.byref(params), L.ptr(w),
                                         C.addressof(res), int(device)))
    return list(res), w[:m]


def _per_candidate(v, n: int, default: float) -> np.ndarray:
    """The reference's rule for kappa / tau: the caller's vector when it has one entry per candidate, else the default."""
    v = np.zeros(0) if v is None else np.atleast_1d(np.asarray(v, dtype=np.float64))
    return v if v.shape == (n,) else np.full(n, float(default))


def robustSingleRotationAveraging(RVec, kappa, errorThreshold: float, device: int = 0):
    """robustSingleRotationAveraging (src/DPGO_solver.cpp:72-135) on the device -> (ROpt, inlierIndices)."""
    tiles = candidate_tiles(RVec)
    m, d = tiles.shape[0], tiles.shape[2]
    prm = average_params(True, errorThreshold, min_inliers=0)
    res, w = robust_average(tiles, prm, _per_candidate(kappa, m, 1.0), None, device=device)
    if res[0].status != L.AVERAGE_OK and res[0].status != L.AVERAGE_FEW_INLIERS:
        raise ValueError("robustSingleRotationAveraging: %s" % L.AVERAGE_STATUS[res[0].status])
    T = np.array(res[0].T[:(d + 1) * d]).reshape(d + 1, d)
    return np.ascontiguousarray(T[:d].T), [int(i) for i in np.nonzero(w > 1 - prm.w_tol)[0]]


def robustSinglePoseAveraging(RVec, tVec, kappa, tau, errorThreshold: float, device: int = 0):
    """robustSinglePoseAveraging (src/DPGO_solver.cpp:137-218) on the device -> (ROpt, tOpt, inlierIndices); kappa / tau
    default to 10000 / 100 as there (:148-149)."""
    tiles = candidate_tiles(RVec, tVec)
    m, d = tiles.shape[0], tiles.shape[2]
    prm = average_params(False, errorThreshold, min_inliers=0)
    res, w = robust_average(tiles, prm, _per_candidate(kappa, m, 10000.0), _per_candidate(tau, m, 100.0), device=device)
    if res[0].status != L.AVERAGE_OK:
        raise ValueError("robustSinglePoseAveraging: %s" % L.AVERAGE_STATUS[res[0].status])
    T = np.array(res[0].T[:(d + 1) * d]).reshape(d + 1, d)
    return np.ascontiguousarray(T[:d].T), T[d].copy(), [int(i) for i in np.nonzero(w > 1 - prm.w_tol)[0]]


def odometry_initialization(odometry: RelativeSEMeasurements, num_poses: int) -> np.ndarray:
    """odometryInitialization: poses composed along the edges p -> p + 1; pose 0 is the identity."""
    d, n = odometry.d, int(num_poses)
    p1, p2, R, t, _, _ = _arrays(odometry)
    T = np.zeros((n, d + 1, d))
    L.check(L.load().dpgo_odometry_initialization(d, n, len(odometry), L.ptr(p1), L.ptr(p2), L.ptr(R), L.ptr(t), L.ptr(T)))
    return T
