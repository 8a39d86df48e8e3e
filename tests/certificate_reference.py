"""numpy / scipy restatement of the certificate of global optimality (include/dpgo_hip.h), used by
tests/test_certificate_*.py:  X is r x (d+1)n (the tile layout), Lambda(X) = blockdiag(Lambda_i) with top-left block
sym(Y_i^T (XQ)_rot,i) and a zero last row / column, C(X) = Q - Lambda(X); the deflation space Z = span(rows of X,
translation indicator)."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def sparse_Q(Qb):
    """oracle BSR -> scipy CSR ((d+1)n x (d+1)n)."""
    N = Qb.n * Qb.b
    return sp.bsr_matrix((Qb.vals.reshape(-1, Qb.b, Qb.b), Qb.colidx, Qb.rowptr), shape=(N, N)).tocsr()


def lambda_blocks(Q, X, d):
    """[n, d, d] blocks sym(Y_i^T (XQ)_rot,i)."""
    r, N = X.shape
    b = d + 1
    n = N // b
    XQ = np.asarray((Q.T @ X.T).T)  # (Q symmetric)
    Y = X.reshape(r, n, b)[:, :, :d]
    G = XQ.reshape(r, n, b)[:, :, :d]
    S = np.einsum("rna,rnc->nac", Y, G)
    return 0.5 * (S + S.transpose(0, 2, 1))


def certificate_matrix(Q, X, d):
    b = d + 1
    S = lambda_blocks(Q, X, d)
    n = S.shape[0]
    L = np.zeros((n, b, b))
    L[:, :d, :d] = S
    return (Q - sp.block_diag(list(L), format="csr")).tocsr()


def certificate_apply(Q, X, V, d):
    """V C(X) without forming C."""
    r, N = V.shape
    b = d + 1
    n = N // b
    S = lambda_blocks(Q, X, d)
    out = np.asarray((Q.T @ V.T).T).copy()
    Vr = V.reshape(r, n, b)[:, :, :d]
    o = out.reshape(r, n, b)
    o[:, :, :d] -= np.einsum("rna,nac->rnc", Vr, S)
    return out


def indicator(n, d):
    t = np.zeros(n * (d + 1))
    t[d::d + 1] = 1.0
    return t


def null_basis(X, d, rtol=1e-10):
    """orthonormal basis of span(rows of X, t), rank-revealing: N x k."""
    n = X.shape[1] // (d + 1)
    K = np.vstack([X, indicator(n, d)[None, :]]).T
    U, s, _ = np.linalg.svd(K, full_matrices=False)
    return U[:, s > rtol * s[0]]


def complement_lambda_min(Cm, Z):
    """dense: smallest eigenvalue of C on the orthogonal complement of span(Z)."""
    N = Cm.shape[0]
    P = np.eye(N) - Z @ Z.T
    U, s, _ = np.linalg.svd(P)
    B = U[:, : N - Z.shape[1]]
    return np.linalg.eigvalsh(B.T @ Cm @ B)[0]


def complement_lambda_min_sparse(Cs, Z, scale, seed=0):
    """scipy LOBPCG with Z as constraints and a shifted sparse-LU preconditioner: smallest eigenvalue of C on Z's
    complement (large problems)."""
    N = Cs.shape[0]
    lu = spla.splu((Cs + 1e-3 * scale * sp.identity(N)).tocsc())
    M = spla.LinearOperator((N, N), matvec=lambda v: lu.solve(np.asarray(v).reshape(-1)), dtype=np.float64)
    rng = np.random.default_rng(seed)
    X0 = rng.standard_normal((N, 4))
    w, _ = spla.lobpcg(Cs, X0, M=M, Y=Z, largest=False, tol=1e-10, maxiter=500)
    return float(np.min(w))


DENSE_LIMIT = 1500  # (d+1)n up to which the dense route is taken (complement_lambda_min's N x N SVD is too slow well below it)


def operator_norm1(Cs):
    """|C|_1 of a sparse matrix: the size of the operator that the suite's 1e-12 scalar tolerance is relative to."""
    return float(abs(Cs).sum(axis=0).max())


def _complement_dense(Cs, Z):
    """(I - Z Z^T) C (I - Z Z^T) + |C|_1 Z Z^T: C on Z's complement, span(Z) moved to the top of the spectrum."""
    Cm = Cs.toarray() if sp.issparse(Cs) else np.asarray(Cs)
    CZ = Cm @ Z
    A = Cm - CZ @ Z.T - Z @ CZ.T + Z @ ((Z.T @ CZ) @ Z.T) + np.abs(Cm).sum(axis=0).max() * (Z @ Z.T)
    return 0.5 * (A + A.T)


def lambda_min_dense(Cs, Z, k=1):
    """The k smallest eigenvalues of C on the orthogonal complement of span(Z) (orthonormal columns), by eigvalsh."""
    return np.linalg.eigvalsh(_complement_dense(Cs, Z))[:k]


def lambda_min_lanczos(Cs, Z, k=1, tol=1e-12, seed=0):
    """The same by eigsh(which="SA") on the projected operator: no factorisation, no deflation beyond Z -- for a C whose
    smallest eigenvalue on the complement is well separated (an arbitrary X), any size."""
    N = Cs.shape[0]
    top = operator_norm1(Cs)

    def mv(v):
        v = np.asarray(v).reshape(-1)
        zv = Z.T @ v
        u = Cs @ (v - Z @ zv)
        return u - Z @ (Z.T @ u) + top * (Z @ zv)

    v0 = np.random.default_rng(seed).standard_normal(N)
    w = spla.eigsh(spla.LinearOperator((N, N), matvec=mv, dtype=np.float64), k=k, which="SA", tol=tol, v0=v0,
                   return_eigenvectors=False)
    return np.sort(w)


def lambda_min(Cs, Z, k=1):
    """Dense up to DENSE_LIMIT rows, Lanczos above."""
    return lambda_min_dense(Cs, Z, k) if Cs.shape[0] <= DENSE_LIMIT else lambda_min_lanczos(Cs, Z, k)


def ring_measurements(oracle, n, d, kappa=1.0):
    """n-pose ring, identity measurements, kappa = tau on every edge (1 unless given)."""
    if kappa != 1.0:
        om, n = ring_measurements(oracle, n, d)
        om.kappa = kappa * om.kappa
        om.tau = kappa * om.tau
        return om, n
    m = n
    z = np.zeros(m, dtype=np.int64)
    p1 = np.arange(n, dtype=np.int64)
    p2 = (p1 + 1) % n
    R = np.repeat(np.eye(d)[None], m, 0)
    return oracle.Measurements(d, z, p1, z.copy(), p2, R, np.zeros((m, d)), np.ones(m), np.ones(m), np.ones(m),
                               np.zeros(m, dtype=bool)), n


def ring_iterate(n, d, r, winding):
    """X (r x (d+1)n): rotation of pose i by 2 pi winding i / n about one axis, translations 0."""
    b = d + 1
    X = np.zeros((r, n * b))
    for i in range(n):
        th = 2 * np.pi * winding * i / n
        Rm = np.eye(d)
        Rm[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
        X[:d, i * b:i * b + d] = Rm
    return X
