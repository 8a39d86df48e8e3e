"""np.longdouble restatement of the GNC re-weighting path (kernels/agent.h: K10 k_edge_robust, K9 k_rebuild_Q; agents.hip:
refresh_after_weights), used by tests/test_reweighting_*.py, with a-priori bounds for the device's fp64 results.  Nothing here
calls the oracle's fp64 code.

Layouts: X and the neighbour tiles are [n, d+1, r] (the tile view of the r x (d+1)n matrix: X[i, :d, :] = Y_i^T, X[i, d, :] =
p_i); block values are [nnzb, d+1, d+1] row-major per block on a block-CSR pattern with sorted columns; edges are any object
with the arrays p1, p2, R [m, d, d], t [m, d], kappa, tau.  role[e] = 0 private, 1 shared outgoing (p1 mine, the other pose =
neighbour tile slot[e]), 2 shared incoming (p2 mine).

Bounds (u = 2^-53, the unit round-off of fp64; every count is the number of roundings a term can pass through in the kernel,
fused multiply-adds counted once; none of them is fitted to a measurement):

* squared residual, c_rsq(d, r) = r d + 2 d + 2 on
      mag = kappa sum (|Y_i R| + |Y_j|)^2 + tau sum (|p_j| + |p_i| + |Y_i| |t|)^2.
  One entry v of Y_i R - Y_j is d FMAs on -Y_j: d roundings, |dv| <= d u V with V its magnitude; v^2 then moves by
  2 |v| |dv| <= 2 d u V^2.  The r d squares are summed by FMAs (<= r d roundings on each), kappa * rot, tau * tr and their
  sum add two more on each term: r d + 2 d + 2.  The translation term needs r + 2 (d + 1) + 2, which is smaller for every
  (d, r) of the library (r (d - 1) >= 2).

* rebuilt block value, c_slot = n_s + (d + 1) + 4 + 1 on
      M = |vals0| + sum over the slot's n_s contributions of (|contrib(w0)| + |contrib(w1)|),
  |contrib| taken TERM BY TERM (sum_k |T_pk| |om_k| |T_qk| for T Om T^T: the rows of a rotation are orthogonal, so the value
  itself cancels where its rounding error does not).  One term is w * kappa (1 rounding), T_pk * om_k (1) and an FMA chain of
  d + 1 links (<= d + 1): d + 3; the slot's sum adds <= n_s roundings to each contribution; base = vals0 - sum adds one on
  |vals0| and one on the w0 contributions; the second pass repeats this on base and the w1 contributions, so that no part of M
  sees more than n_s + (d + 1) + 4 roundings.  The last + 1 covers this reference's own arithmetic (2^-64 per operation, i.e.
  2^-11 u each) and the conversion of its result to fp64 for the comparison.

* a product with rebuilt values: sum_j (c_slot u M_ij) |V_j|, plus the suite's own tolerance for Q V (1e-13 relative,
  tests/test_launch_geometry_gpu.py), both in the Frobenius norm (product_bound).
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
QV_RTOL = 1e-13  # the suite's tolerance for Q V against an exact product (tests/test_launch_geometry_gpu.py)


def _ld(a):
    return np.asarray(a, dtype=LD)


def _i64(a):
    return np.asarray(a, dtype=np.int64)


def roles_and_slots(meas, my_id):
    """(role, slot, slots) of one agent's edges (r1, r2 = robot ids): slots = the sorted (robot, frame) ids of the
    neighbours' poses = the order of the neighbour tile buffer."""
    r1, r2, p1, p2 = _i64(meas.r1), _i64(meas.r2), _i64(meas.p1), _i64(meas.p2)
    m = len(p1)
    role = np.zeros(m, dtype=np.uint8)
    ids = []
    for e in range(m):
        if r1[e] != r2[e]:
            role[e] = 1 if r1[e] == my_id else 2
            ids.append((int(r2[e]), int(p2[e])) if role[e] == 1 else (int(r1[e]), int(p1[e])))
    slots = sorted(set(ids))
    index = {pid: k for k, pid in enumerate(slots)}
    slot = np.zeros(m, dtype=np.int32)
    slot[role != 0] = [index[pid] for pid in ids]
    return role, slot, slots


def _edge_tiles(meas, X, nbr, role, slot):
    X = _ld(X)
    m = len(meas.p1)
    role = np.zeros(m, dtype=np.uint8) if role is None else np.asarray(role)
    p1, p2 = _i64(meas.p1), _i64(meas.p2)
    xi = X[np.where(role == 2, 0, p1)]
    xj = X[np.where(role == 1, 0, p2)]
    if (role != 0).any():
        nbr, slot = _ld(nbr), _i64(slot)
        xi[role == 2] = nbr[slot[role == 2]]
        xj[role == 1] = nbr[slot[role == 1]]
    return xi, xj


def residuals(meas, X, nbr=None, role=None, slot=None):
    """rSq = kappa |Y_i R - Y_j|_F^2 + tau |p_j - p_i - Y_i t|^2 of every edge, the pose a neighbour owns taken from
    nbr[slot] (roles 1, 2).  Returns (rsq, mag): mag the magnitude the bound c_rsq u mag refers to (module docstring)."""
    d = np.asarray(meas.R).shape[-1]
    if len(meas.p1) == 0:
        return np.zeros(0, dtype=LD), np.zeros(0, dtype=LD)
    xi, xj = _edge_tiles(meas, X, nbr, role, slot)
    Yi, Yj = np.swapaxes(xi[:, :d, :], 1, 2), np.swapaxes(xj[:, :d, :], 1, 2)  # [m, r, d]
    pi, pj = xi[:, d, :], xj[:, d, :]
    R, t = _ld(meas.R), _ld(meas.t)
    YR = np.einsum("mak,mkc->mac", Yi, R)
    Yt = np.einsum("mak,mk->ma", Yi, t)
    kappa, tau = _ld(meas.kappa), _ld(meas.tau)
    rsq = kappa * np.sum((YR - Yj) ** 2, axis=(1, 2)) + tau * np.sum((pj - pi - Yt) ** 2, axis=1)
    aYt = np.einsum("mak,mk->ma", np.abs(Yi), np.abs(t))
    mag = kappa * np.sum((np.abs(YR) + np.abs(Yj)) ** 2, axis=(1, 2)) + \
        tau * np.sum((np.abs(pj) + np.abs(pi) + aYt) ** 2, axis=1)
    return rsq, mag


def c_rsq(d, r):
    return r * d + 2 * d + 2


def rsq_bound(mag, d, r):
    return c_rsq(d, r) * U * _ld(mag)


def tls_weight_fp64(rsq, mu, barc):
    """The GNC-TLS weight as k_edge_robust and the reference library evaluate it, in fp64 and in their order of
    operations: r = sqrt(rsq), rSq = r r, >= upper -> 0, <= lower -> 1, else sqrt(bSq mu (mu + 1) / rSq) - mu."""
    rsq = np.asarray(rsq, dtype=np.float64)
    mu, barc = np.float64(mu), np.float64(barc)
    r = np.sqrt(rsq)
    rSq, bSq = r * r, barc * barc
    upper, lower = (mu + 1.0) / mu * bSq, mu / (mu + 1.0) * bSq
    with np.errstate(divide="ignore", invalid="ignore"):
        mid = np.sqrt(bSq * mu * (mu + 1.0) / rSq) - mu
    return np.where(rSq >= upper, 0.0, np.where(rSq <= lower, 1.0, mid))


def tls_thresholds(mu, barc):
    """(lower, upper) in fp64, as the kernel forms them."""
    mu, barc = np.float64(mu), np.float64(barc)
    bSq = barc * barc
    return mu / (mu + 1.0) * bSq, (mu + 1.0) / mu * bSq


def tls_parameters_for(rsq_free, lo=0.3, hi=0.7):
    """(mu, barc) whose thresholds are the lo and hi quantiles of the given residuals: lower = mu / (mu + 1) barc^2,
    upper = (mu + 1) / mu barc^2, so upper / lower = ((mu + 1) / mu)^2 and lower upper = barc^4."""
    q = np.quantile(np.asarray(rsq_free, dtype=np.float64), [lo, hi])
    s = float(np.sqrt(q[1] / q[0]))
    return 1.0 / (s - 1.0), float((q[0] * q[1]) ** 0.25)


def tls_branches(rsq, mu, barc):
    """0 (weight 1), 1 (between the thresholds), 2 (weight 0) per edge."""
    lower, upper = tls_thresholds(mu, barc)
    r = np.sqrt(np.asarray(rsq, dtype=np.float64))
    return np.where(r * r >= upper, 2, np.where(r * r <= lower, 0, 1))


# ---------------------------------------------------------------- values-only rebuild
def contributions(meas, w):
    """Per edge the four blocks an edge adds (kind 0: T Om T^T, 1: Om, 2: -T Om, 3: -Om T^T; T = [R t; 0 1], Om =
    w diag(kappa.., tau)) and their term-by-term magnitudes: ([m, b, b] x 4, [m, b, b] x 4)."""
    R, t = _ld(meas.R), _ld(meas.t)
    m, d = R.shape[0], R.shape[-1]
    b = d + 1
    T = np.zeros((m, b, b), dtype=LD)
    T[:, :d, :d] = R
    T[:, :d, d] = t
    T[:, d, d] = 1
    om = np.empty((m, b), dtype=LD)
    om[:, :d] = (_ld(w) * _ld(meas.kappa))[:, None]
    om[:, d] = _ld(w) * _ld(meas.tau)
    TO = T * om[:, None, :]
    Om = np.zeros((m, b, b), dtype=LD)
    Om[:, np.arange(b), np.arange(b)] = om
    aTO = np.abs(TO)
    vals = (np.einsum("mpk,mqk->mpq", TO, T), Om, -TO, -np.swapaxes(TO, 1, 2))
    mags = (np.einsum("mpk,mqk->mpq", aTO, np.abs(T)), np.abs(Om), aTO, np.swapaxes(aTO, 1, 2))
    return vals, mags


def find_slots(rowptr, colidx, ncols, rows, cols):
    """Positions of the blocks (rows, cols) in a block-CSR pattern with sorted columns."""
    rowptr, colidx = _i64(rowptr), _i64(colidx)
    key = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)) * ncols + colidx
    want = _i64(rows) * ncols + _i64(cols)
    pos = np.searchsorted(key, want)
    assert (pos < len(key)).all() and (key[np.minimum(pos, len(key) - 1)] == want).all(), "block not in the pattern"
    return pos


def q_targets(meas, role=None):
    """[(edges, kind, block row, block column)] of Q: a private edge i -> j adds kind 0 to (i, i), 1 to (j, j), 2 to (i, j),
    3 to (j, i); a shared outgoing edge kind 0 to (i, i), a shared incoming one kind 1 to (j, j)."""
    p1, p2 = _i64(meas.p1), _i64(meas.p2)
    role = np.zeros(len(p1), dtype=np.uint8) if role is None else np.asarray(role)
    e0, e1, e2 = (np.nonzero(role == k)[0] for k in (0, 1, 2))
    return [(e0, 0, p1[e0], p1[e0]), (e0, 1, p2[e0], p2[e0]), (e0, 2, p1[e0], p2[e0]), (e0, 3, p2[e0], p1[e0]),
            (e1, 0, p1[e1], p1[e1]), (e2, 1, p2[e2], p2[e2])]


def c_targets(meas, role, slot):
    """... of the coupling blocks: outgoing C(i, slot) = -T Om, incoming C(j, slot) = -Om T^T."""
    p1, p2, slot, role = _i64(meas.p1), _i64(meas.p2), _i64(slot), np.asarray(role)
    e1, e2 = np.nonzero(role == 1)[0], np.nonzero(role == 2)[0]
    return [(e1, 2, p1[e1], slot[e1]), (e2, 3, p2[e2], slot[e2])]


def _scatter_add(out, s, vals):
    """out[s] += vals with repeated slots (np.add.at, but fast on large edge lists): sorted by slot, summed per run."""
    order = np.argsort(s, kind="stable")
    uniq, first = np.unique(s[order], return_index=True)
    out[uniq] += np.add.reduceat(vals[order], first, axis=0)


def _rebuilt(rowptr, colidx, ncols, vals0, meas, w0, w1, targets):
    K0, A0 = contributions(meas, w0)
    K1, A1 = contributions(meas, w1)
    base = _ld(vals0).copy()
    M = np.abs(base)
    count = np.zeros(len(base), dtype=np.int64)
    where = [(e, kind, find_slots(rowptr, colidx, ncols, rows, cols)) for e, kind, rows, cols in targets if len(e)]
    for e, kind, s in where:
        _scatter_add(base, s, -K0[kind][e])
        _scatter_add(M, s, A0[kind][e] + A1[kind][e])
        _scatter_add(count, s, np.ones(len(s), dtype=np.int64))
    out = base.copy()
    for e, kind, s in where:
        _scatter_add(out, s, K1[kind][e])
    return out, M, count


def rebuilt_Q(rowptr, colidx, vals0, meas, w0, w1, role=None):
    """The two-step scheme on Q's values: base = vals0 - sum contributions(w0), result = base + sum contributions(w1).
    Returns (result, M, count): M = |vals0| + sum (|contrib(w0)| + |contrib(w1)|) element-wise, count = contributions per
    slot."""
    return _rebuilt(rowptr, colidx, len(rowptr) - 1, vals0, meas, w0, w1, q_targets(meas, role))


def rebuilt_C(rowptr, colidx, ncols, vals0, meas, w0, w1, role, slot):
    """The same for the coupling blocks (n x ncols block pattern)."""
    return _rebuilt(rowptr, colidx, ncols, vals0, meas, w0, w1, c_targets(meas, role, slot))


def c_slot(count, d):
    return np.asarray(count, dtype=np.int64) + (d + 1) + 4 + 1


def value_bound(M, count, d):
    """c_slot u M per element of the rebuilt values."""
    return c_slot(count, d)[:, None, None] * (U * _ld(M))


def block_product(rowptr, colidx, vals, V):
    """out[i] = sum_s vals[s] V[colidx[s]] over block row i: Q V, or the neighbours' part of G, in the tile view."""
    rowptr, colidx = _i64(rowptr), _i64(colidx)
    V = _ld(V)
    n = len(rowptr) - 1
    out = np.zeros((n,) + V.shape[1:], dtype=LD)
    if len(colidx):
        prod = np.einsum("spq,sqr->spr", _ld(vals), V[colidx])
        _scatter_add(out, np.repeat(np.arange(n), np.diff(rowptr)), prod)
    return out


def product_bound(rowptr, colidx, E, V, want):
    """Frobenius-norm bound of a device product with rebuilt values against `want`: |sum_j E_ij |V_j|| for the values'
    element-wise bound E, plus the suite's tolerance for the product itself."""
    e = block_product(rowptr, colidx, E, np.abs(_ld(V)))
    return float(np.sqrt(np.sum(e * e))) + QV_RTOL * float(np.sqrt(np.sum(_ld(want) ** 2)))


def fro(a):
    a = _ld(a)
    return float(np.sqrt(np.sum(a * a)))
