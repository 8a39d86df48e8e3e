"""fp64 numpy restatement of the team staircase step (include/dpgo_hip.h: dpgo_team_eval_device,
dpgo_team_escape_device; DESIGN.md section 10, "Team staircase"), on the CENTRAL Q of oracle.construct_Q: what a team
computes from its pieces is the central problem's f, rgrad and S.  X is r x (d+1)n (the tile layout) throughout."""
import numpy as np

import certificate_reference as ref
from certificate_cases import matrix_of, tiles_of


def team_eval(Q, X, d):
    """(f, rgrad, S): f = 0.5 <X Q, X>, S_i = sym(Y_i^T (XQ)_rot,i) [n, d, d], rgrad_i = (XQ)_i - [Y_i S_i, 0]
    (r x (d+1)n)."""
    r, N = X.shape
    b = d + 1
    n = N // b
    XQ = np.asarray((Q.T @ X.T).T)  # (Q symmetric)
    S = ref.lambda_blocks(Q, X, d)
    rg = XQ.copy()
    rg.reshape(r, n, b)[:, :, :d] -= np.einsum("rna,nac->rnc", X.reshape(r, n, b)[:, :, :d], S)
    return 0.5 * float(np.sum(XQ * X)), rg, S


def lift_retract(oracle, X, w, alpha, d):
    """qf([X; alpha w^T]): (r + 1) x (d+1)n, by oracle.qf_retract on the lifted tiles."""
    Xl = np.vstack([X, alpha * np.asarray(w, dtype=np.float64).reshape(1, -1)])
    Xt = tiles_of(Xl, d)
    return matrix_of(oracle.qf_retract(Xt, np.zeros_like(Xt), d))


def escape(oracle, Q, X, w, d, grad_tol):
    """SE-Sync's rule: f0 at alpha = 0, alpha = 0.1 sqrt(n) 2^-k for k = 0 .. 59, the first with f < f0 and
    |rgrad| > grad_tol.  dict(alpha, k, f_before, f_after, gradnorm_after, X) or None."""
    n = X.shape[1] // (d + 1)
    f0 = team_eval(Q, X, d)[0]
    for k in range(60):
        alpha = 0.1 * np.sqrt(n) * 0.5 ** k
        Xn = lift_retract(oracle, X, w, alpha, d)
        f, rg, _ = team_eval(Q, Xn, d)
        gn = float(np.linalg.norm(rg))
        if f < f0 and gn > grad_tol:
            return dict(alpha=alpha, k=k, f_before=f0, f_after=f, gradnorm_after=gn, X=Xn)
    return None


def dense_witness(Q, X, d):
    """(lambda_min, w): the smallest eigen-pair of C(X) on the complement of span(rows of X, t), dense; w a unit
    vector."""
    Z = ref.null_basis(X, d)
    lam, V = np.linalg.eigh(ref._complement_dense(ref.certificate_matrix(Q, X, d), Z))
    w = V[:, 0] - Z @ (Z.T @ V[:, 0])
    return float(lam[0]), w / np.linalg.norm(w)
