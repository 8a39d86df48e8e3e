"""References and seeded inputs for the agent layer's device kernels (csrc/agents.hip, csrc/kernels/agent.h): the pose
movers (k_gather_tiles, k_scatter_tiles, k_gather_tiles_batched), the coupling product G = G0 + Xnbr C (k_spmm on the
rectangular block-CSR operator of dpgo_problem_set_G_coupling), the relative change of the iterate
(k_max_translation_distance) and the block-Jacobi factors (k_build_dinv).

NumPy only.  Whatever involves arithmetic runs in np.longdouble (the 80-bit format, asserted by manifold_reference);
the pose movers are plain indexing.  The input generators live here too, so that the CPU test can check that every case
holds what its name claims (tests/test_agent_layer_reference_cpu.py) before tests/test_agent_layer_gpu.py relies on it.

Layouts: a pose is a tile [d+1, r] (the bytes of the r x (d+1) column-major lifted pose); block t of a block-CSR
operator is vals[t], (d+1) x (d+1) row-major, and row i of the product is sum_t vals[t] @ V[colidx[t]].
"""
import numpy as np

import manifold_reference as M

LD = M.LD
U = 2.0 ** -53  # unit roundoff of fp64
DR = M.DR
GRID_CAP = 1024  # kMaxGrid (kernels/common.h)
BLOCK = 256      # kBlock


# ---------------------------------------------------------------- pose movers
def gather(src, idx):
    """out[k] = src[idx[k]] (k_gather_tiles; dpgo_permute_tiles_device with forward = 0)."""
    return np.asarray(src)[np.asarray(idx, dtype=np.int64)]


def scatter(src, idx):
    """out[idx[k]] = src[k], idx a permutation (k_scatter_tiles; dpgo_permute_tiles_device with forward = 1)."""
    src = np.asarray(src)
    out = np.empty_like(src)
    out[np.asarray(idx, dtype=np.int64)] = src
    return out


def exchange(messages):
    """[(src, idx), ...] -> [src[idx], ...] (k_gather_tiles_batched: one launch, every message)."""
    return [gather(s, i) for s, i in messages]


# ---------------------------------------------------------------- block-CSR product
def coupling_G(G0, rowptr, colidx, vals, Xnbr):
    """(G, mag): G = G0 + Xnbr C in longdouble, tiles [n, d+1, r], G[i] = G0[i] + sum_t vals[t] @ Xnbr[colidx[t]] over
    the blocks t of row i; mag = |G0| + |Xnbr| |C|, the componentwise magnitude the forward error bound multiplies.
    G0 None: zero.  Xnbr [ncols, d+1, r] carries the shape when there is no block."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    n = len(rowptr) - 1
    b, r = Xnbr.shape[1], Xnbr.shape[2]
    G = np.zeros((n, b, r), dtype=LD) if G0 is None else np.array(G0, dtype=LD).reshape(n, b, r)
    mag = np.abs(G)
    if len(colidx):
        rows = np.repeat(np.arange(n), np.diff(rowptr))
        V = np.array(vals, dtype=LD).reshape(-1, b, b)
        X = np.array(Xnbr, dtype=LD)[colidx]
        np.add.at(G, rows, np.einsum("tck,tka->tca", V, X))
        np.add.at(mag, rows, np.einsum("tck,tka->tca", np.abs(V), np.abs(X)))
    return G, mag


def row_terms(rowptr, b):
    """k of the forward error bound, per row: (d + 1) x (blocks in that row) fma terms."""
    return b * np.diff(np.asarray(rowptr, dtype=np.int64))


def tangent_project(X, W, d):
    """Stiefel::ExtrProjection per pose in longdouble (tiles): the rotation rows lose Y sym(Y^T W); the translation row
    stays."""
    X, W = np.array(X, dtype=LD), np.array(W, dtype=LD)
    Y, Wy = X[:, :d, :], W[:, :d, :]
    S = np.einsum("nak,nck->nac", Y, Wy)
    S = (S + np.swapaxes(S, 1, 2)) / 2
    out = W.copy()
    out[:, :d, :] = Wy - np.einsum("nac,nak->nck", S, Y)
    return out


def eval_terms(Q, G, Gmag, X, d):
    """(sum(XQ . X), sum(X . G), |rgrad|^2) in longdouble with the magnitude sums of the first two (what the scalar
    tolerance multiplies).  Q: an oracle BSR; G, Gmag from coupling_G."""
    QX, QXmag = coupling_G(None, Q.rowptr, Q.colidx, Q.vals, X)
    Xl = np.array(X, dtype=LD)
    xqx, xg = np.sum(Xl * QX), np.sum(Xl * G)
    rg = tangent_project(X, QX + G, d)
    return (xqx, xg, np.sum(rg * rg)), (np.sum(np.abs(Xl) * QXmag), np.sum(np.abs(Xl) * Gmag))


# ---------------------------------------------------------------- relative change
def max_translation_distance(X, Xprev):
    """LiftedPoseArray::maxTranslationDistance in longdouble: max_i |p_i - p_i'|, p the last row of a tile."""
    dlt = np.array(np.asarray(X)[:, -1, :], dtype=LD) - np.array(np.asarray(Xprev)[:, -1, :], dtype=LD)
    return np.sqrt(np.sum(dlt * dlt, axis=1)).max()


# ---------------------------------------------------------------- small inverses
def block_inverse(A):
    """[n, b, b] -> inverses, Gauss-Jordan with partial pivoting in longdouble (manifold_reference's)."""
    return M._inv(A)


# ================================================================ seeded inputs
def tile_poses(d, split):
    """Poses per workgroup tile of a <D, R, SPLIT> kernel (Geo::P, kernels/common.h)."""
    return 4 * (64 // ((d + 1) * split))


def tiles(rng, n, T):
    """n distinct tiles of T doubles whose bits identify (tile, element): a misplaced element cannot pass."""
    return rng.standard_normal((n, T)) + np.arange(n)[:, None]


# ---- A. pose movers
GATHER_COUNTS = (1, 63, 64, 65, 257)


def gather_big_count(T):
    """A count whose element total exceeds GRID_CAP * BLOCK (the grid-stride trip of k_gather_tiles): 11 000 tiles at
    T = 24, scaled."""
    return 11000 * 24 // T + 1


def gather_indices(n, count, seed):
    """count indices into n tiles: index 0, index n - 1 and a duplicate are among them whenever count allows."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n, count).astype(np.int32)
    fixed = [n - 1, 0, n // 2, n // 2][:count]
    idx[rng.permutation(count)[:len(fixed)]] = fixed
    return idx


EXCHANGE_TABLES = ("one", "two_overlap", "seven_empties", "forty")


def exchange_table(name, seed=0):
    """(source sizes, [(source, idx)]) of one exchange phase.
    one: a single message; two_overlap: two messages that read overlapping poses of one source; seven_empties: empty
    messages in first, middle (two in a row) and last position around messages of one tile; forty: 40 messages from five
    sources, some empty; big: more than 64 * GRID_CAP tiles in total (the grid-stride trip of k_gather_tiles_batched),
    with an empty message between the two long ones; all_empty: total zero."""
    rng = np.random.default_rng(1000 + seed)
    i32 = lambda a: np.asarray(a, dtype=np.int32)
    if name == "one":
        return [9], [(0, i32([3, 0, 8, 3, 5]))]
    if name == "two_overlap":
        return [12], [(0, i32([0, 4, 5, 6, 11])), (0, i32([5, 6, 7, 4]))]
    if name == "seven_empties":
        return [6, 3], [(0, i32([])), (1, i32([2])), (0, i32([])), (1, i32([])), (0, i32([5, 0, 5])), (1, i32([0])),
                        (0, i32([]))]
    if name == "forty":
        sizes = [17, 1, 64, 5, 33]
        msgs = []
        for m in range(40):
            s = m % 5
            cnt = 0 if m in (3, 4, 22) else int(rng.integers(1, 10))
            msgs.append((s, i32(rng.integers(0, sizes[s], cnt))))
        return sizes, msgs
    if name == "big":
        sizes = [5000, 777]
        return sizes, [(0, gather_indices(5000, 40000, seed)), (1, i32([])), (1, gather_indices(777, 25637, seed + 1)),
                       (0, i32([4999]))]
    if name == "all_empty":
        return [4], [(0, i32([])), (0, i32([])), (0, i32([]))]
    raise KeyError(name)


# ---- B. coupling patterns
def coupling_pattern(n, ncols, d, seed):
    """(rowptr, colidx, info) of a rectangular n x ncols block pattern, column indices sorted and unique per row.
    ncols = 0: no block.  ncols = 1: about two rows in three hold the one possible block.  Otherwise, from 4 rows on:
    rows 0 and n - 1 and about every fifth row in between are empty; slot 0 is a hub that every other row references (60
    rows at least from n = 100 on); with ncols >= d + 4 one row holds (d + 1) + 3 blocks, with ncols >= 4 (d + 1) + 3
    another holds that many (more than the preloaded index window of every split); the rest hold 1 to 3 blocks.
    info: empty (rows), hub_degree, long_rows {row: blocks}."""
    rng = np.random.default_rng(seed)
    b = d + 1
    info = {"empty": [], "hub_degree": 0, "long_rows": {}}
    cand = np.zeros((n, 4), dtype=np.int64)  # per row: the hub column, then up to three more, sorted
    take = np.zeros((n, 4), dtype=bool)
    long_cols = {}
    if ncols == 1:
        take[:, 0] = rng.random(n) < 0.66
        if n >= 3:
            take[0, 0] = take[n - 1, 0] = False
            take[1, 0] = True
        else:
            take[:, 0] = True
    elif ncols > 1:
        empty = rng.random(n) < 0.2
        if n >= 4:
            empty[0] = empty[n - 1] = True
            empty[1] = empty[2] = False
        else:
            empty[:] = False
        more = rng.integers(0, min(3, ncols - 1) + 1, n)
        draw = rng.integers(1, ncols, (n, 3))
        draw[np.arange(3)[None, :] >= more[:, None]] = ncols  # (not drawn)
        draw.sort(axis=1)
        fresh = np.ones((n, 3), dtype=bool)
        fresh[:, 1:] = draw[:, 1:] != draw[:, :-1]
        cand[:, 1:] = draw
        take[:, 0] = True
        take[:, 1:] = (draw < ncols) & fresh
        take[empty] = False
        busy = np.nonzero(~empty)[0]
        for blocks in (b + 3, 4 * b + 3):
            free = [i for i in busy if i not in long_cols]
            if ncols >= blocks and free:
                i = int(free[len(free) // 2])
                long_cols[i] = np.sort(rng.choice(ncols, blocks, replace=False))
                info["long_rows"][i] = blocks
                take[i] = False
    deg = take.sum(axis=1)
    for i, c in long_cols.items():
        deg[i] = len(c)
    rowptr = np.zeros(n + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(deg)
    colidx = np.zeros(rowptr[-1], dtype=np.int32)
    short = np.ones(rowptr[-1], dtype=bool)
    for i, c in long_cols.items():
        colidx[rowptr[i]:rowptr[i + 1]] = c
        short[rowptr[i]:rowptr[i + 1]] = False
    colidx[short] = cand[take]
    info["empty"] = [int(i) for i in np.nonzero(deg == 0)[0]]
    info["hub_degree"] = int(np.sum(colidx == 0))
    return rowptr, colidx, info


def coupling_big_n(d, split):
    """The smallest convenient pose count whose tile count exceeds GRID_CAP (k_spmm's tile walk takes a second trip):
    16 400 poses at d = 3 and 20 600 at d = 2 for split 4; a tile and 16 poses past the cap for the other splits."""
    if split == 4:
        return {3: 16400, 2: 20600}[d]
    P = tile_poses(d, split)
    return GRID_CAP * P + P + 16


def coupling_pose_counts(d, split):
    P = tile_poses(d, split)
    return sorted({1, P - 1, P, P + 1, 17 * P + 3}) + [coupling_big_n(d, split)]


# ---- C. relative change
CHANGE_COUNTS = (1, 63, 64, 65, 255, 256, 257, GRID_CAP * BLOCK, GRID_CAP * BLOCK + 1)
CHANGE_PLACES = ("first", "last", "wave_end", "second_trip")


def change_place(n, place):
    """The pose that holds the maximum, or None where the place does not exist at n poses: pose 0, pose n - 1, lane 63 of
    the first wave, the first pose of the second grid-stride trip."""
    i = {"first": 0, "last": n - 1, "wave_end": 63, "second_trip": GRID_CAP * BLOCK}[place]
    return i if i < n else None


def change_base(d, r, n, seed):
    """(X, Xprev): tiles whose translation distances are all at most 0.5; the rotation rows differ arbitrarily."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d + 1, r))
    Xp = rng.standard_normal((n, d + 1, r))
    step = rng.standard_normal((n, r))
    step *= (rng.uniform(0.0, 0.5, n) / np.linalg.norm(step, axis=1))[:, None]
    Xp[:, d, :] = X[:, d, :] - step
    return X, Xp


def change_peak(X, at, seed):
    """The translation row of Xprev[at] that puts pose `at` at distance 1 (to rounding): twice every distance of
    change_base."""
    step = np.random.default_rng(seed).standard_normal(X.shape[2])
    return X[at, -1, :] - step / np.linalg.norm(step)


def change_case(d, r, n, at, seed):
    """(X, Xprev) of change_base with the maximum put at pose `at`."""
    X, Xp = change_base(d, r, n, seed)
    Xp[at, d, :] = change_peak(X, at, seed + 1)
    return X, Xp


# ---- E. block-Jacobi factors
JACOBI_VALUES = (1.0, 1e4, 1e8)
JACOBI_CLASS_EDGES = (1e2, 1e6)  # kappa_2 below 1e2 / up to 1e6 / above: the blocks cluster at 1e0-1e1, 1e4 and 1e8


def jacobi_graph(d, n, seed):
    """Edge arrays (p1, p2, R, t, kappa, tau) of a small pose graph whose diagonal blocks span the conditioning classes: an
    odometry chain and n / 2 loop closures; the poses are cut into three runs, and an edge that leaves a pose of run c has
    kappa and tau drawn from {1, JACOBI_VALUES[c]}; the last pose has 60 edges more (as many as there are other poses, if
    fewer)."""
    rng = np.random.default_rng(seed)
    pairs = [(i, i + 1) for i in range(n - 1)]
    seen = set(pairs)
    while len(pairs) < n - 1 + n // 2 and n >= 4:
        i, j = sorted(int(v) for v in rng.integers(0, n, 2))
        if j > i + 1 and (i, j) not in seen:
            seen.add((i, j))
            pairs.append((i, j))
    hub = n - 1
    for o in rng.permutation(n - 2)[:60]:
        if (int(o), hub) not in seen:
            seen.add((int(o), hub))
            pairs.append((hub, int(o)))
    p1 = np.array([p[0] for p in pairs], dtype=np.int32)
    p2 = np.array([p[1] for p in pairs], dtype=np.int32)
    m = len(pairs)
    if d == 2:
        a = rng.uniform(-np.pi, np.pi, m)
        R = np.stack([np.stack([np.cos(a), -np.sin(a)], 1), np.stack([np.sin(a), np.cos(a)], 1)], 1)
    else:
        q = rng.standard_normal((m, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        w, x, y, z = q.T
        R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1),
                      np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], 1),
                      np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)
    t = rng.standard_normal((m, d))
    cls = np.minimum(3 * p1.astype(np.int64) // max(n, 1), 2)
    big = np.asarray(JACOBI_VALUES)[cls]
    kappa = np.where(rng.random(m) < 0.5, 1.0, big)
    tau = np.where(rng.random(m) < 0.5, 1.0, big)
    return p1, p2, np.ascontiguousarray(R), np.ascontiguousarray(t), kappa, tau


def condition_class(A):
    """Class 0, 1, 2 of every symmetric positive definite block [n, b, b] by its 2-norm condition number (fp64
    eigenvalues: the classes are decades apart), and the condition numbers."""
    w = np.linalg.eigvalsh(np.asarray(A, dtype=np.float64))
    k2 = w[:, -1] / w[:, 0]
    return np.digitize(k2, JACOBI_CLASS_EDGES), k2


def inverse_error(inv, exact):
    """Per block: max |inv - exact| / max |exact|."""
    exact = np.array(exact, dtype=LD)
    err = np.abs(np.array(inv, dtype=LD) - exact).max(axis=(1, 2)) / np.abs(exact).max(axis=(1, 2))
    return err.astype(np.float64)


def axis_frames(d, r, n, seed):
    """(X, axis): per pose a Stiefel point whose d columns are signed coordinate axes of R^r, and one axis more that is
    orthogonal to them (r > d).  Every product against them is exact, so block-Jacobi of a V whose columns are multiples of
    that axis passes the tangent projection unchanged, bit for bit."""
    assert r > d
    rng = np.random.default_rng(seed)
    X = np.zeros((n, d + 1, r))
    axis = np.zeros(n, dtype=np.int64)
    for i in range(n):
        p = rng.permutation(r)
        X[i, np.arange(d), p[:d]] = rng.choice([-1.0, 1.0], d)
        axis[i] = p[d]
    X[:, d, :] = rng.standard_normal((n, r))
    return X, axis
