"""tests/agent_layer_reference.py pinned without a GPU: its longdouble references against the oracle, and every input
generator against what its case claims (tests/test_agent_layer_gpu.py relies on both)."""
import ctypes as C
import os

import numpy as np
import pytest

import agent_layer_reference as A
from conftest import DATA, matrix_to_tiles

DR = A.DR


def test_pose_movers_are_plain_indexing():
    rng = np.random.default_rng(0)
    src = A.tiles(rng, 7, 6)
    idx = np.array([6, 0, 3, 3], dtype=np.int32)
    got = A.gather(src, idx)
    assert got.shape == (4, 6) and all(np.array_equal(got[k], src[idx[k]]) for k in range(4))
    perm = rng.permutation(7).astype(np.int32)
    fwd = A.scatter(src, perm)
    assert all(np.array_equal(fwd[perm[k]], src[k]) for k in range(7))
    assert np.array_equal(A.gather(fwd, perm), src)  # the inverse direction undoes the forward one
    out = A.exchange([(src, idx), (fwd, perm[:0])])
    assert np.array_equal(out[0], got) and out[1].shape == (0, 6)
    assert len(np.unique(A.tiles(rng, 300, 24))) == 300 * 24  # no two elements alike: a misplaced one shows


def test_coupling_G_matches_the_oracle(oracle):
    """coupling_G on the coupling operator of every agent of smallGrid3D split into 5 (the data of
    test_multi_agent_G_and_local_problem) against oracle.construct_G.  Both sum the same products, the oracle in fp64:
    twice the device bound (k + 2) 2^-53 mag covers its roundings and those of the operator's values."""
    import dpgo_amd
    r = 5
    om, n = oracle.read_g2o(os.path.join(DATA, "smallGrid3D.g2o"))
    d = om.d
    ranges, per = oracle.partition_contiguous(om, n, 5)
    dataset, _ = dpgo_amd.read_g2o_file(os.path.join(DATA, "smallGrid3D.g2o"))
    _, per_p = dpgo_amd.partition_contiguous(dataset, n, 5)
    X = oracle.polar_project(np.random.default_rng(3).standard_normal((n, d + 1, r)), d)
    blocks = 0
    for a in range(5):
        s, e = ranges[a]
        pg = dpgo_amd.PoseGraph(a, r, d)
        pg.setMeasurements(per_p[a])
        nbr = {(rob, fr): X[ranges[rob][0] + fr] for (rob, fr) in pg.neighborPoseIDs()}
        want = oracle.construct_G(e - s, d, r, per[a]["shared"], a, nbr)
        slots, rowptr, colidx, vals, G0 = pg.couplingMatrix()
        Xnbr = np.stack([nbr[sid] for sid in slots])
        G, mag = A.coupling_G(matrix_to_tiles(G0, d), rowptr, colidx, vals, Xnbr)
        assert G.dtype == A.LD and G.shape == want.shape == mag.shape
        k = A.row_terms(rowptr, d + 1)[:, None, None]
        assert np.all(np.abs(G - want) <= 2 * (k + 2) * A.U * mag), a
        assert np.all(G[k[:, 0, 0] == 0] == 0)
        blocks += len(colidx)
    assert blocks > 50


def test_coupling_G_shapes_without_blocks():
    G0 = np.random.default_rng(1).standard_normal((3, 4, 5))
    G, mag = A.coupling_G(G0, np.zeros(4, dtype=np.int32), np.zeros(0, dtype=np.int32), None, np.zeros((0, 4, 5)))
    assert np.array_equal(G.astype(np.float64), G0) and np.array_equal(mag.astype(np.float64), np.abs(G0))
    G, mag = A.coupling_G(None, np.zeros(4, dtype=np.int32), np.zeros(0, dtype=np.int32), None, np.zeros((0, 3, 2)))
    assert G.shape == (3, 3, 2) and not G.any() and not mag.any()


def test_eval_terms_match_the_oracle(oracle):
    """eval_terms (the longdouble (XQX, X.G, |rgrad|^2) of the concurrent-evaluation test) against the oracle's fp64
    QuadraticProblem on a random graph with a linear term, to the parity suite's scalar tolerance."""
    from test_parity_gpu import _random_graph
    d, r, n = 3, 5, 30
    om, T, _ = _random_graph(oracle, d, n, 10, 5, seed=4)
    Q = oracle.construct_Q(n, d, om)
    rng = np.random.default_rng(5)
    X = oracle.polar_project(oracle.lift(T, r) + 0.1 * rng.standard_normal((n, d + 1, r)), d)
    G = rng.standard_normal((n, d + 1, r))
    op = oracle.QuadraticProblem(Q, G, r, d)
    (xqx, xg, g2), (mq, mg) = A.eval_terms(Q, np.array(G, dtype=A.LD), np.abs(G), X, d)
    assert abs(float(0.5 * xqx + xg) - op.f(X)) <= 1e-12 * float(0.5 * mq + mg)
    assert abs(float(np.sqrt(g2)) - op.rie_grad_norm(X)) <= 1e-12 * op.rie_grad_norm(X)
    assert mq >= abs(xqx) and mg >= abs(xg)


@pytest.mark.parametrize("d,r", DR)
def test_max_translation_distance_matches_the_oracle(oracle, d, r):
    for n in (1, 65, 300):
        X, Xp = A.change_case(d, r, n, n // 2, seed=n + r)
        want = oracle.max_translation_distance(X, Xp)
        got = A.max_translation_distance(X, Xp)
        assert got.dtype == A.LD
        assert abs(float(got) - want) <= (r + 2) * A.U * want
    assert A.max_translation_distance(X, X) == 0


def test_block_inverse_times_block_is_the_identity():
    """On the blocks of part E, both dimensions and both shifts: |inv A - I| <= 64 eps_longdouble kappa_2(A)."""
    for d in (2, 3):
        for shift in (0.1, 1e-3):
            blocks = _jacobi_blocks(d, A.tile_poses(d, 1) + 1, shift)
            inv = A.block_inverse(blocks)
            assert inv.dtype == A.LD
            _, k2 = A.condition_class(blocks)
            res = np.abs(inv @ np.array(blocks, dtype=A.LD) - np.eye(d + 1, dtype=A.LD)).max(axis=(1, 2))
            assert np.all(res <= 64 * float(np.finfo(A.LD).eps) * k2), (d, shift, float((res / k2).max()))
            assert np.all(A.inverse_error(inv, inv) == 0)


# ---------------------------------------------------------------- the generators
def test_gather_indices_hold_duplicates_and_both_ends():
    for T in (6, 9, 12, 15, 16, 20, 24):
        big = A.gather_big_count(T)
        assert big * T > A.GRID_CAP * A.BLOCK and (big - 600) * T < A.GRID_CAP * A.BLOCK
        for count in A.GATHER_COUNTS + (big,):
            n = count + 37
            idx = A.gather_indices(n, count, seed=count)
            assert idx.dtype == np.int32 and len(idx) == count and idx.min() >= 0 and idx.max() < n
            if count >= 4:
                assert 0 in idx and n - 1 in idx and len(np.unique(idx)) < count


def test_exchange_tables_hold_what_they_claim():
    counts = {}
    for name in A.EXCHANGE_TABLES + ("big", "all_empty"):
        sizes, msgs = A.exchange_table(name)
        for s, idx in msgs:
            assert idx.dtype == np.int32 and (len(idx) == 0 or (idx.min() >= 0 and idx.max() < sizes[s]))
        counts[name] = [len(idx) for _, idx in msgs]
    assert [len(counts[k]) for k in A.EXCHANGE_TABLES] == [1, 2, 7, 40]
    c = counts["seven_empties"]
    assert c[0] == 0 and c[-1] == 0 and c[2] == c[3] == 0 and c[1] == 1 and c[5] == 1 and c[4] > 1
    sizes, msgs = A.exchange_table("two_overlap")
    assert msgs[0][0] == msgs[1][0] and len(set(msgs[0][1]) & set(msgs[1][1])) >= 2
    assert counts["forty"].count(0) >= 3 and counts["forty"][3] == counts["forty"][4] == 0 and 1 in counts["forty"]
    assert len({s for s, _ in A.exchange_table("forty")[1]}) == 5
    big = counts["big"]
    assert sum(big) > 64 * A.GRID_CAP and big[0] < 64 * A.GRID_CAP and 0 in big  # (the second trip crosses a message)
    assert sum(big) * 6 * 8 < 4 << 20
    assert sum(counts["all_empty"]) == 0 and len(counts["all_empty"]) > 1


@pytest.mark.parametrize("d", [2, 3])
def test_coupling_patterns_hold_what_they_claim(d):
    b = d + 1
    for split in (1, 2, 4):
        counts = A.coupling_pose_counts(d, split)
        P = A.tile_poses(d, split)
        assert counts[-1] > A.GRID_CAP * P >= counts[-1] - 4 * P - 400 and counts[-2] == 17 * P + 3
        for n in counts:
            ncols = max(4 * b + 3, n // 3)
            rowptr, colidx, info = A.coupling_pattern(n, ncols, d, seed=n)
            assert rowptr[0] == 0 and rowptr[-1] == len(colidx) and np.all(np.diff(rowptr) >= 0)
            for i in range(n):
                row = colidx[rowptr[i]:rowptr[i + 1]]
                assert np.all(np.diff(row) > 0) and (len(row) == 0 or (row[0] >= 0 and row[-1] < ncols))
            deg = np.diff(rowptr)
            assert info["empty"] == list(np.nonzero(deg == 0)[0])
            if n >= 4:
                assert 0 in info["empty"] and n - 1 in info["empty"]
            else:
                assert not info["empty"]
            assert info["hub_degree"] == np.sum(colidx == 0) >= min(60, n - len(info["empty"]) - 2)
            if n >= 100:
                assert info["hub_degree"] >= 60
            if n >= 8:
                assert sorted(info["long_rows"].values()) == [b + 3, 4 * b + 3]
            for i, blocks in info["long_rows"].items():
                assert deg[i] == blocks
            # one column: a block or none; no column: none
            rowptr, colidx, info = A.coupling_pattern(n, 1, d, seed=n)
            assert set(np.diff(rowptr)) <= {0, 1} and not colidx.any() and len(colidx) >= 1
            if n >= 3:
                assert 0 in info["empty"] and n - 1 in info["empty"]
            rowptr, colidx, info = A.coupling_pattern(n, 0, d, seed=n)
            assert not rowptr.any() and len(colidx) == 0 and len(info["empty"]) == n


def test_relative_change_cases_put_the_maximum_where_they_say():
    d, r = 2, 3
    assert A.CHANGE_COUNTS[-2] == A.GRID_CAP * A.BLOCK
    for n in A.CHANGE_COUNTS:
        X, Xp = A.change_base(d, r, n, seed=n)
        dist = np.linalg.norm(X[:, d, :] - Xp[:, d, :], axis=1)
        assert dist.max() <= 0.5 * (1 + 1e-12)
        places = [p for p in A.CHANGE_PLACES if A.change_place(n, p) is not None]
        assert "first" in places and "last" in places
        assert ("wave_end" in places) == (n >= 64) and ("second_trip" in places) == (n > A.GRID_CAP * A.BLOCK)
        for p in places:
            at = A.change_place(n, p)
            row = A.change_peak(X, at, seed=7)
            others = np.delete(dist, at)
            peak = np.linalg.norm(X[at, d, :] - row)
            assert abs(peak - 1.0) < 1e-12 and (len(others) == 0 or others.max() <= 0.5 * peak * (1 + 1e-12))
    X, Xp = A.change_case(d, r, 300, 63, seed=1)
    dist = np.linalg.norm(X[:, d, :] - Xp[:, d, :], axis=1)
    assert np.argmax(dist) == 63 and not np.array_equal(X[:, :d, :], Xp[:, :d, :])


def _jacobi_blocks(d, n, shift):
    """The diagonal blocks Q_ii + shift I of jacobi_bsr."""
    return jacobi_bsr(d, n)[3] + shift * np.eye(d + 1)


def jacobi_bsr(d, n):
    """(rowptr, colidx, vals, diagonal blocks) of Q on jacobi_graph through dpgo_build_Q_bsr (host code)."""
    import dpgo_amd.lib as L
    lib = L.load()
    p1, p2, R, t, kappa, tau = A.jacobi_graph(d, n, seed=11 + d)
    m = len(p1)
    z, w = np.zeros(m, dtype=np.int32), np.ones(m)
    args = [0, d, n, m, L.ptr(z), L.ptr(p1), L.ptr(z), L.ptr(p2), L.ptr(R), L.ptr(t), L.ptr(kappa), L.ptr(tau), L.ptr(w), 0,
            None, 0.0, 0.0]
    nnzb = C.c_int(0)
    L.check(lib.dpgo_build_Q_bsr(*args, C.byref(nnzb), None, None, None))
    rowptr, colidx = np.zeros(n + 1, dtype=np.int32), np.zeros(nnzb.value, dtype=np.int32)
    vals = np.zeros((nnzb.value, d + 1, d + 1))
    L.check(lib.dpgo_build_Q_bsr(*args, C.byref(nnzb), L.ptr(rowptr), L.ptr(colidx), L.ptr(vals)))
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    diag = vals[rows == colidx]
    assert len(diag) == n
    return rowptr, colidx, vals, diag


@pytest.mark.parametrize("d", [2, 3])
def test_jacobi_graph_spans_the_conditioning_classes(d):
    n = A.tile_poses(d, 1) + 1
    p1, p2, R, t, kappa, tau = A.jacobi_graph(d, n, seed=11 + d)
    assert np.sum((p1 == n - 1) | (p2 == n - 1)) >= 60  # the pose of degree 60
    assert set(np.unique(kappa)) == set(A.JACOBI_VALUES) == set(np.unique(tau))
    assert np.allclose(R @ np.swapaxes(R, 1, 2), np.eye(d)) and np.allclose(np.linalg.det(R), 1.0)
    for shift in (0.1, 1e-3):
        blocks = _jacobi_blocks(d, n, shift)
        skew = np.abs(blocks - np.swapaxes(blocks, 1, 2)).max(axis=(1, 2))  # (symmetric to the rounding of T Om T^T)
        assert np.all(skew <= 1e-15 * np.abs(blocks).max(axis=(1, 2)))
        cls, k2 = A.condition_class(blocks)
        assert all(np.sum(cls == c) >= 5 for c in range(3)), np.bincount(cls)
        assert 1e7 < k2.max() < 1e10 and k2.min() < 1e1


@pytest.mark.parametrize("d,r", [(2, 3), (3, 4), (3, 6)])
def test_axis_frames_are_exactly_orthonormal(d, r):
    X, axis = A.axis_frames(d, r, 40, seed=2)
    Y = X[:, :d, :]
    assert np.array_equal(Y @ np.swapaxes(Y, 1, 2), np.broadcast_to(np.eye(d), (40, d, d)))
    u = np.zeros((40, r))
    u[np.arange(40), axis] = 1.0
    assert not np.einsum("nak,nk->na", Y, u).any() and len(set(axis)) > 1
