"""The NumPy restatement of the robust frame alignment (tests/frame_alignment_reference.py) against the reference's own
tests (tests/testPGO.cpp:14-128), and what the GPU tests rely on for every committed input: the planted inlier set is the
one found, and the fp64 and the longdouble run agree in inlier set and iteration count."""
import numpy as np
import pytest

import frame_alignment_reference as F
from manifold_reference import LD

TRIALS = 12  # (the reference runs 50 of each; the restatement is the same code every time)


def _rng(k):
    return np.random.Generator(np.random.PCG64(1000 + k))


def test_chi2_constant():
    """cbar of the pose mode (src/PGOAgent.cpp:630): sqrt(chi2inv(0.9, 3))."""
    from scipy import stats
    assert abs(stats.chi2.ppf(0.9, 3) - F.CHI2INV_09_3) <= 1e-13
    assert abs(F.angular2chordal(0.5) - 2 * np.sqrt(2) * np.sin(0.25)) == 0.0


def test_rotation_averaging_trivial():
    """tests/testPGO.cpp:14-30: one candidate is its own average and an inlier."""
    for k in range(TRIALS):
        Rtrue = F.random_rotations(_rng(k), 1, 3)
        out = F.robust_single_rotation_averaging(Rtrue, 1.0, F.angular2chordal(0.5))
        assert np.linalg.norm(out["R"] - Rtrue[0]) <= 1e-8
        assert list(out["inliers"]) == [0] and out["iterations"] == 0


def test_rotation_averaging_with_outliers():
    """tests/testPGO.cpp:32-60: 10 exact inliers, 40 outliers further than 1.2 cbar, cbar = angular2ChordalSO3(0.3)."""
    tol, cbar = F.angular2chordal(0.02), F.angular2chordal(0.3)
    for k in range(TRIALS):
        rng = _rng(100 + k)
        Rtrue = F.random_rotations(rng, 1, 3)[0]
        Rs = [Rtrue] * 10
        while len(Rs) < 50:
            Rr = F.random_rotations(rng, 1, 3)[0]
            if np.linalg.norm(Rr - Rtrue) > 1.2 * cbar:
                Rs.append(Rr)
        out = F.robust_single_rotation_averaging(np.array(Rs), np.ones(50), cbar)
        assert np.linalg.norm(out["R"] - Rtrue) <= tol
        assert list(out["inliers"]) == list(range(10))


def test_pose_averaging_trivial():
    """tests/testPGO.cpp:62-84."""
    cbar = np.sqrt(F.CHI2INV_09_3)
    for k in range(TRIALS):
        Rtrue = F.random_rotations(_rng(200 + k), 1, 3)
        out = F.robust_single_pose_averaging(Rtrue, np.zeros((1, 3)), 10000.0, 100.0, cbar)
        assert np.linalg.norm(out["R"] - Rtrue[0]) <= 1e-8 and np.linalg.norm(out["t"]) <= 1e-8
        assert list(out["inliers"]) == [0]


def test_pose_averaging_with_outliers():
    """tests/testPGO.cpp:86-128: kappa 10 000, tau 100, translations of the outliers uniform in [-1, 1]^3."""
    cbar, kappa, tau = np.sqrt(F.CHI2INV_09_3), 10000.0, 100.0
    for k in range(TRIALS):
        rng = _rng(300 + k)
        Rtrue = F.random_rotations(rng, 1, 3)[0]
        Rs, ts = [Rtrue] * 10, [np.zeros(3)] * 10
        while len(Rs) < 50:
            Rr, tr = F.random_rotations(rng, 1, 3)[0], rng.uniform(-1, 1, 3)
            if np.sqrt(kappa * np.sum((Rtrue - Rr) ** 2) + tau * np.sum(tr ** 2)) > 1.2 * cbar:
                Rs.append(Rr), ts.append(tr)
        out = F.robust_single_pose_averaging(np.array(Rs), np.array(ts), np.full(50, kappa), np.full(50, tau), cbar)
        assert np.linalg.norm(out["R"] - Rtrue) <= F.angular2chordal(0.02)
        assert np.linalg.norm(out["t"]) <= 1e-2
        assert list(out["inliers"]) == list(range(10))


@pytest.mark.parametrize("mode", [F.TWO_STAGE, F.POSE])
@pytest.mark.parametrize("d", [2, 3])
def test_committed_inputs_are_decidable(d, mode):
    """Every group the GPU test runs: the planted set is found, fp64 and longdouble agree in inlier set and iterations, and
    the fp64 estimate is within rounding of the longdouble one."""
    case, r64, rld = F.reference_runs(d, mode)
    gp = case["group_ptr"]
    assert [int(gp[g + 1] - gp[g]) for g in range(len(gp) - 1)] == [n for _, n in F.GROUP_SIZES]
    for g, (a, b) in enumerate(zip(r64, rld)):
        planted = np.nonzero(case["planted"][gp[g]:gp[g + 1]])[0]
        assert len(planted) == F.GROUP_SIZES[g][0]
        assert list(a["inliers"]) == list(planted), (g, a["inliers"], planted)
        assert list(b["inliers"]) == list(planted), g
        assert a["iterations"] == b["iterations"], (g, a["iterations"], b["iterations"])
        assert a["status"] == b["status"] == (F.OK if len(planted) >= 2 else F.FEW_INLIERS)
        decided = (b["weights"] < F.W_TOL) | (b["weights"] > 1 - F.W_TOL)
        assert decided.all()
        err = max(np.max(np.abs(a["R"] - b["R"])), np.max(np.abs(a["t"] - b["t"])) / 10.0)
        assert float(err) <= 1e-13, (g, float(err))
        if mode == F.TWO_STAGE:  # (the pose mode returns its LAST solve, which still carries the outliers' last weights)
            Rtrue, ttrue = case["truth"][g]
            assert np.linalg.norm(np.asarray(b["t"], dtype=np.float64) - ttrue) <= 0.05


def test_unit_weights_are_pulled_by_outliers():
    """The same input averaged without GNC is far from the truth: the inputs can tell a robust average from a plain one."""
    case, r64, _ = F.reference_runs(3, F.POSE)
    gp = case["group_ptr"]
    g = len(gp) - 2
    R, t = case["R"][gp[g]:gp[g + 1]], case["t"][gp[g]:gp[g + 1]]
    plain = F.robust_transform(R, t, F.POSE, unit_weights=True)
    assert np.linalg.norm(plain["t"] - case["truth"][g][1]) > 1.0
    assert np.linalg.norm(r64[g]["t"] - case["truth"][g][1]) <= 0.5


@pytest.mark.parametrize("d,r", [(2, 3), (3, 5)])
def test_candidates_and_lift_are_consistent(d, r):
    """A neighbour that holds the lifted ground truth and exact measurements: every candidate is the true transform from my
    frame to the world, in both edge directions, and the lifted local trajectory is the lifted truth."""
    rng = _rng(400 + d)
    n, slots, m = 7, 9, 20
    Y = np.linalg.qr(rng.standard_normal((r, d)))[0]
    Rw, tw = F.random_rotations(rng, 1, d)[0], rng.uniform(-5, 5, d)  # world <- my frame
    Rl, tl = F.random_rotations(rng, n, d), rng.uniform(-5, 5, (n, d))  # my poses in my frame
    Rn, tn = F.random_rotations(rng, slots, d), rng.uniform(-5, 5, (slots, d))  # neighbour poses in the world
    Xn = F.lift_in_frame(Y, F.to_tiles(np.eye(d)[None], np.zeros((1, d)))[0], F.to_tiles(Rn, tn), LD)
    my, sl, inc = rng.integers(0, n, m), rng.integers(0, slots, m), rng.integers(0, 2, m)
    Rmine, tmine = F.se_compose(Rw[None], tw[None], Rl[my], tl[my])  # my poses in the world
    # measurement p1 -> p2: inv(T_p1) T_p2, p1 mine for an outgoing edge
    Ro, to = F.se_compose(*F.se_inverse(Rmine, tmine), Rn[sl], tn[sl])
    Ri, ti = F.se_compose(*F.se_inverse(Rn[sl], tn[sl]), Rmine, tmine)
    Re, te = np.where(inc[:, None, None] == 1, Ri, Ro), np.where(inc[:, None] == 1, ti, to)
    cand = F.neighbor_transforms(Y, Xn, F.to_tiles(Rl, tl), my, sl, inc, Re, te, LD)
    want = F.to_tiles(Rw[None], tw[None])[0]
    assert float(np.max(np.abs(cand - want[None]))) <= 1e-13
    X = F.lift_in_frame(Y, want, F.to_tiles(Rl, tl), LD)
    Rall, tall = F.se_compose(Rw[None], tw[None], Rl, tl)
    Xtrue = F.lift_in_frame(Y, F.to_tiles(np.eye(d)[None], np.zeros((1, d)))[0], F.to_tiles(Rall, tall), LD)
    assert float(np.max(np.abs(X - Xtrue))) <= 1e-13
