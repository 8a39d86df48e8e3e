"""Case table for the certificate of global optimality (a plain module, no tests): dpgo_problem_certify*,
dpgo_certify_escape_device, csrc/certify.hip, csrc/kernels/certify.h against tests/certificate_reference.py.

C(X) = Q - Lambda(X) is defined at ANY X on the manifold.  At an arbitrary X only the translation indicator t is null
(C t = 0 exactly: Lambda has a zero last row and column, Q t = 0), C is strongly indefinite and its smallest eigenvalue is
well separated, so a dense or Lanczos eigen-solver gives the reference without any deflation and the device gets there in
tens of iterations.  tests/test_certificate_cases_cpu.py checks every margin named here on the reference alone; where a
seed misses one, SEEDS holds another -- the expected values are never changed to fit.

A. every (d, r) x pose counts around the workgroup tile x {unit, random} kappa / tau, X = polar_project(Gaussian):
   NOT_CERTIFIED, one deflated direction.
B. twisted rings (stationary, analytic lambda_min = kappa (-2 (1 - cos 2 pi / n)), d + 1 deflated directions), winding 0
   (CERTIFIED at + |lambda_ring|), scaled weights, a turned X, three seeds, three preconditioners.
C. eta is relative to scale and two-sided.
D. a NOT_CERTIFIED verdict is a proof even when the budget ends (max_iterations 1, 2, 5).
E. deflation follows the documented rule (|C z| against sqrt(tol_rel) scale) on a perturbed ring.
F. big blocks: second trips of the grid-stride loops.
G. dpgo_problem_certify_device and dpgo_certify_escape_device.
H. tiny graphs.

Iteration budgets: max_iterations = max(200, 4 x the count of restatement() -- the documented iteration in numpy) (the
device's start block is a hash, numpy's a generator, and the count moves with the start block).  The counts are recorded
below (A_ITS, RING_ITS, ...) as upper bounds that the CPU test holds the restatement to.
"""
from dataclasses import dataclass

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

import certificate_reference as ref

DR = [(2, 2), (2, 3), (2, 4), (2, 5), (3, 3), (3, 4), (3, 5), (3, 6)]  # DPGO_FOR_DR (csrc/host.h)
LIFTS = [(d, r) for d, r in DR if (d, r + 1) in DR]  # every r -> r + 1 that dpgo_supported allows
TOL_REL, ETA = 1e-9, 1e-6
GAP = 1e-3  # (lambda_2 - lambda_1) / scale of groups A and F
SCALAR_TOL = 1e-12  # the suite's tolerance of a scalar, relative to the size of the operator


def tile_poses(d, split=1):
    """Poses per workgroup tile of a <D, R, SPLIT> kernel (Geo::P, kernels/common.h)."""
    return 4 * (64 // ((d + 1) * split))


# (d+1) n = 64 + 2 (2-D) / 64 + 4 (3-D): the second 64-column chunk of k_cert_gram holds the fewest columns it can
RAGGED = {2: 22, 3: 17}


def budget(count):
    return max(200, 4 * count)


def matrix_of(Xt):
    """[n, d+1, r] tiles -> r x (d+1)n."""
    n, b, r = Xt.shape
    return np.ascontiguousarray(Xt).reshape(n * b, r).T


def tiles_of(X, d):
    r, N = X.shape
    return np.ascontiguousarray(np.asfortranarray(X).T).reshape(N // (d + 1), d + 1, r)


# ---------------------------------------------------------------- problems (cached per module)
_GRAPHS = {}


def random_graph(oracle, d, n, unit):
    """(om, Qb, Qs): _random_graph (chain, n / 2 loop closures, a hub row), kappa / tau random in [5, 50] or all 1."""
    key = ("graph", d, n, unit)
    if key not in _GRAPHS:
        from test_parity_gpu import _random_graph
        om, _, _ = _random_graph(oracle, d, n, n // 2, 40 if n >= 64 else max(0, n - 4) // 2, seed=900 + 10 * n + d)
        if unit:
            om.kappa, om.tau = np.ones_like(om.kappa), np.ones_like(om.tau)
        Qb = oracle.construct_Q(n, d, om)
        _GRAPHS[key] = (om, Qb, ref.sparse_Q(Qb))
    return _GRAPHS[key]


def chain_graph(oracle, d, n):
    """n >= 2 poses, odometry only."""
    key = ("chain", d, n)
    if key not in _GRAPHS:
        from test_parity_gpu import _random_graph
        om, T, _ = _random_graph(oracle, d, n, 0, 0, seed=40 + 10 * n + d)
        Qb = oracle.construct_Q(n, d, om)
        _GRAPHS[key] = (om, Qb, ref.sparse_Q(Qb), T)
    return _GRAPHS[key]


def ring_graph(oracle, d, n, kappa=1.0):
    key = ("ring", d, n, kappa)
    if key not in _GRAPHS:
        om, _ = ref.ring_measurements(oracle, n, d, kappa)
        Qb = oracle.construct_Q(n, d, om)
        _GRAPHS[key] = (om, Qb, ref.sparse_Q(Qb))
    return _GRAPHS[key]


def lattice_graph(oracle, dims):
    """"NXxNY": _grid2d_measurements (seed 4); "NXxNYxNZ": oracle.synthetic_grid (seed 0)."""
    key = ("lattice", dims)
    if key not in _GRAPHS:
        sizes = [int(v) for v in dims.split("x")]
        if len(sizes) == 2:
            from test_parity_gpu import _grid2d_measurements
            om, n = _grid2d_measurements(oracle, *sizes, seed=4)
        else:
            om, n, _ = oracle.synthetic_grid(*sizes, seed=0)
        Qb = oracle.construct_Q(n, om.d, om)
        _GRAPHS[key] = (om, Qb, ref.sparse_Q(Qb))
    return _GRAPHS[key]


def random_iterate(oracle, n, d, r, seed):
    """polar_project of a Gaussian: a point of the manifold that is nowhere near stationary."""
    return matrix_of(oracle.polar_project(np.random.default_rng(seed).standard_normal((n, d + 1, r)), d))


class Instance:
    """A problem and an iterate with everything numpy knows about C(X)."""

    def __init__(self, om, Qb, Qs, X):
        self.om, self.Qb, self.Q, self.X = om, Qb, Qs, np.ascontiguousarray(X)
        self.d, self.r, self.n = om.d, X.shape[0], Qb.n
        self.C = ref.certificate_matrix(Qs, self.X, self.d)
        self.scale = float(Qs.diagonal().max())
        self.eps = SCALAR_TOL * ref.operator_norm1(self.C)
        self._ref = {}

    def null_tol(self, tol_rel=TOL_REL):
        return np.sqrt(tol_rel) * self.scale

    def gradnorm(self, oracle):
        return oracle.QuadraticProblem(self.Qb, None, self.r, self.d, precond="none").rie_grad_norm(tiles_of(self.X, self.d))

    def row_space_residuals(self):
        """|C z| over an orthonormal basis z of span(rows of X) that diagonalises it: the singular values of C B,
        ascending."""
        U, s, _ = np.linalg.svd(self.X.T, full_matrices=False)
        B = U[:, s > 1e-10 * s[0]]
        return np.sort(np.linalg.svd(self.C @ B, compute_uv=False))

    def Z(self, deflated):
        """What the documented rule deflates: t alone (an X that is not stationary), or span(rows of X, t)."""
        if deflated == 1:
            return (ref.indicator(self.n, self.d) / np.sqrt(self.n))[:, None]
        Z = ref.null_basis(self.X, self.d)
        assert Z.shape[1] == deflated, (Z.shape, deflated)
        return Z

    def documented_Z(self, tol_rel=TOL_REL):
        """(Z, clear): the rule of include/dpgo_hip.h for any X -- of span(rows of X, t), the directions z with
        |C z| <= sqrt(tol_rel) scale.  clear = no |C z| within a factor 10 of that threshold and no singular value of
        [X; t] between 1e-10 and 1e-4 of the largest (where the rank-revealing cut may fall either way)."""
        K = np.vstack([self.X, ref.indicator(self.n, self.d)[None, :]]).T
        U, s, _ = np.linalg.svd(K, full_matrices=False)
        B = U[:, s > 1e-7 * s[0]]
        _, sig, Vt = np.linalg.svd(self.C @ B, full_matrices=False)
        clear = not np.any((s > 1e-10 * s[0]) & (s < 1e-4 * s[0]))
        clear = clear and not np.any((sig > 0.1 * self.null_tol(tol_rel)) & (sig < 10 * self.null_tol(tol_rel)))
        return B @ Vt[sig <= self.null_tol(tol_rel)].T, clear

    def lambdas(self, deflated, k=2):
        """The k smallest eigenvalues of C on Z(deflated)'s complement (cached)."""
        if (deflated, k) not in self._ref:
            self._ref[(deflated, k)] = ref.lambda_min(self.C, self.Z(deflated), k)
        return self._ref[(deflated, k)]

    def lambda_ref(self, deflated):
        return float(self.lambdas(deflated)[0])

    def jacobi(self, shift=0.1):
        """V -> (blockdiag(Q) + shift I)^-1 V, the device's block-Jacobi preconditioner without tangent projection."""
        b = self.d + 1
        Qc = self.Q.tocsr()
        inv = [np.linalg.inv(Qc[i * b:(i + 1) * b, i * b:(i + 1) * b].toarray() + shift * np.eye(b)) for i in range(self.n)]
        M = sp.block_diag(inv, format="csr")
        return lambda V: M @ V


# ---------------------------------------------------------------- the documented iteration, in numpy
def restatement(Cs, Z, r, tol, precond=None, max_iterations=3000, seed=0):
    """Block LOBPCG of include/dpgo_hip.h on [W, T, P] with blocks of r vectors on the complement of Z (orthonormal
    columns), stopped by the residual of the FIRST Ritz pair: (iterations, theta_0, w_0, converged).  P is dropped for a
    step where the basis is dependent (the device: a Cholesky pivot ratio under 1e-7)."""
    def off(V, U):
        return V - U @ (U.T @ V)

    rng = np.random.default_rng(seed)
    W = np.linalg.qr(off(rng.uniform(-1, 1, (Cs.shape[0], r)), Z))[0]
    theta, U = np.linalg.eigh(W.T @ (Cs @ W))
    W, P = W @ U, None
    for it in range(max_iterations + 1):
        R = Cs @ W - W * theta
        if np.linalg.norm(R[:, 0]) <= tol:
            return it, float(theta[0]), W[:, 0], True
        if it == max_iterations:
            break
        T = off(off(R if precond is None else precond(R), Z), W)
        while True:
            S = np.hstack([W, T] + ([] if P is None else [P]))
            S = S / np.linalg.norm(S, axis=0)
            G = S.T @ S
            if np.linalg.cond(G) < 1e14:
                break
            if P is None:
                return it, float(theta[0]), W[:, 0], False  # T depends on W: stagnated
            P = None
        w, V = sla.eigh(S.T @ (Cs @ S), G)
        Y = V[:, :r]
        W, P, theta = S @ Y, S[:, r:] @ Y[r:], w[:r]
    return max_iterations, float(theta[0]), W[:, 0], False


# ---------------------------------------------------------------- the derived bounds
def witness_figures(inst, Z, lam, w):
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    Cw = inst.C @ w
    return {"norm": abs(np.linalg.norm(w) - 1.0), "ortho": float(np.linalg.norm(Z.T @ w)), "rq": abs(float(w @ Cw) - lam),
            "rho": float(np.linalg.norm(Cw - lam * w))}


def check_pair(inst, Z, lam, w, lam_ref, converged, tol_rel=TOL_REL, label=""):
    """The returned pair (lam, w) against numpy's C.  With rho = |C w - lam w|_2 and eps = 1e-12 |C|_1:
      | |w| - 1 | <= 1e-10, |Z^T w| <= 1e-10, |w^T C w - lam| <= 1e-10 scale;
      a converged run has rho <= tol_rel scale + eps;
      -eps <= lam - lam_ref (a Rayleigh quotient on the complement is not below its minimum), and for a converged run
      lam - lam_ref <= rho + eps (some eigenvalue lies within rho of lam: this fails exactly when it is not the smallest).
    Never the device's own residual."""
    f = witness_figures(inst, Z, lam, w)
    print("%s lam %.12e ref %.12e  | |w|-1 | %.1e  |Z^T w| %.1e  |wCw-lam|/scale %.1e  rho/scale %.2e  eps/scale %.1e" % (
        label, lam, lam_ref, f["norm"], f["ortho"], f["rq"] / inst.scale, f["rho"] / inst.scale, inst.eps / inst.scale))
    assert np.isfinite(lam) and np.isfinite(np.asarray(w)).all()
    assert f["norm"] <= 1e-10 and f["ortho"] <= 1e-10, f
    assert f["rq"] <= 1e-10 * inst.scale, f
    assert lam - lam_ref >= -inst.eps, (lam, lam_ref, inst.eps)
    if converged:
        assert f["rho"] <= tol_rel * inst.scale + inst.eps, f
        assert lam - lam_ref <= f["rho"] + inst.eps, (lam, lam_ref, f)
    return f


# ---------------------------------------------------------------- A. arbitrary iterates
@dataclass(frozen=True)
class Arbitrary:
    d: int
    r: int
    n: int
    unit: bool

    @property
    def name(self):
        return "%d-%d-n%d-%s" % (self.d, self.r, self.n, "unit" if self.unit else "random")


def arbitrary_sizes(d):
    P = tile_poses(d)
    return [RAGGED[d], P - 1, P, P + 1, 17 * P + 3]


A_CASES = [Arbitrary(d, r, n, unit) for d, r in DR for n in arbitrary_sizes(d) for unit in (True, False)]
# case -> seed of its iterate where the first choice (1000 + 17 n + r) misses a margin of the CPU test; behind each entry:
# what the first choice missed
SEEDS = {Arbitrary(3, 5, 1091, True): 20552}  # gap 7.9e-4 of scale
A_ITS = 50  # restatement iterations of every A case at precond = none (seen: 9 - 48): the budget is 200
# the two cases run again with block-Jacobi: an SPD preconditioner of Q is the wrong tool at the strongly negative end of an
# indefinite C, and the count shows it -- restatement iterations (upper bound; seen: 262, 170)
A_JACOBI = {Arbitrary(2, 3, 83, False): 290, Arbitrary(3, 5, 63, True): 190}


def arbitrary(oracle, case):
    om, Qb, Qs = random_graph(oracle, case.d, case.n, case.unit)
    return Instance(om, Qb, Qs, random_iterate(oracle, case.n, case.d, case.r, SEEDS.get(case, 1000 + 17 * case.n + case.r)))


# ---------------------------------------------------------------- B. rings
@dataclass(frozen=True)
class Ring:
    d: int
    r: int
    n: int
    kappa: float = 1.0
    turned: bool = False  # X replaced by A X, A a random orthogonal r x r matrix: C is the same, no row of X is zero

    @property
    def name(self):
        return "%d-%d-n%d%s%s" % (self.d, self.r, self.n, "" if self.kappa == 1.0 else "-kappa%g" % self.kappa,
                                  "-turned" if self.turned else "")


def ring_sizes(d):
    P = tile_poses(d)
    return [P - 1, P + 1, 200, 257]


def ring_lambda(case):
    return case.kappa * (-2.0 * (1.0 - np.cos(2.0 * np.pi / case.n)))


B_CASES = [Ring(d, r, n) for d, r in DR for n in ring_sizes(d)]
B_SCALED = [Ring(2, 3, 85, kappa=7.5), Ring(3, 4, 65, kappa=7.5)]
B_TURNED = [Ring(2, 4, 85, turned=True), Ring(3, 5, 65, turned=True), Ring(3, 3, 63, turned=True)]
B_SEEDED = Ring(3, 4, 65)  # seeds 1, 3, 12345
B_PRECONDS = [Ring(d, r, n) for d, r in [(2, 3), (3, 5)] for n in (200, 257)]  # jacobi and multilevel must agree
RING_PARAMS = dict(eta=ETA, tol_rel=TOL_REL, precond="jacobi", seed=3)
# restatement iterations by pose count, both windings, every (d, r), "none" and block-Jacobi (upper bound)
# (seen at most: 151, 161, 183, 199, 521, 614)
RING_ITS = {63: 170, 65: 180, 83: 205, 85: 220, 200: 580, 257: 680}


def ring(oracle, case, winding=1):
    om, Qb, Qs = ring_graph(oracle, case.d, case.n, case.kappa)
    X = ref.ring_iterate(case.n, case.d, case.r, winding)
    if case.turned:
        X = np.linalg.qr(np.random.default_rng(29 + case.r).standard_normal((case.r, case.r)))[0] @ X
    return Instance(om, Qb, Qs, X)


# ---------------------------------------------------------------- C. the threshold
# (ring, eta, verdict): lambda / scale = -4.67e-3 at n = 65, -4.93e-4 at n = 200
C_CASES = [(Ring(d, r, n), eta, verdict) for d, r in [(2, 3), (3, 4)]
           for n, eta, verdict in [(65, 1e-2, "CERTIFIED"), (65, 1e-3, "NOT_CERTIFIED"), (200, 1e-3, "CERTIFIED"),
                                   (200, 1e-4, "NOT_CERTIFIED")]]

# ---------------------------------------------------------------- D. budgets that end first
D_BUDGETS = (1, 2, 5)
D_CASES = [Arbitrary(d, r, tile_poses(d) + 1, False) for d, r in DR] + [Ring(d, r, tile_poses(d) + 1) for d, r in DR]


# ---------------------------------------------------------------- E. deflation
@dataclass(frozen=True)
class Perturbed:
    """X_eps = qf_retract(X_ring, eps V), V a fixed random tangent vector of unit norm per pose on average."""
    d: int
    r: int
    n: int
    eps: float
    deflated: int

    @property
    def name(self):
        return "%d-%d-n%d-eps%g" % (self.d, self.r, self.n, self.eps)


# r = d: span(rows of X) keeps its dimension d whatever eps is (for r > d the rows that eps V adds to the zero rows of the
# ring iterate are cut or kept by the rank-revealing threshold, which the contract leaves open)
# |C z| / null_tol over the row space: 19 - 32 at eps = 1e-3, 1.9e-4 - 3.2e-4 at eps = 1e-8
E_CASES = [Perturbed(2, 2, 65, 1e-3, 1), Perturbed(2, 2, 65, 1e-8, 3), Perturbed(3, 3, 65, 1e-3, 1),
           Perturbed(3, 3, 65, 1e-8, 4)]
E_ITS = 210  # restatement iterations (upper bound; seen: 142 - 184)


def perturbed(oracle, case):
    om, Qb, Qs = ring_graph(oracle, case.d, case.n)
    Xt = tiles_of(ref.ring_iterate(case.n, case.d, case.r, 1), case.d)
    V = oracle.tangent_project(Xt, np.random.default_rng(71).standard_normal(Xt.shape), case.d)
    V *= np.sqrt(case.n) / np.linalg.norm(V)
    return Instance(om, Qb, Qs, matrix_of(oracle.qf_retract(Xt, case.eps * V, case.d)))


# ---------------------------------------------------------------- F. big blocks
@dataclass(frozen=True)
class Big:
    dims: str
    r: int
    its: int  # restatement iterations (upper bound; the largest takes the count of the 21^3 lattice)
    variants: tuple = ("auto",)

    @property
    def name(self):
        return "%s-r%d" % (self.dims, self.r)


F_CASES = [Big("110x100", 3, 35), Big("21x21x21", 4, 65), Big("41x41x40", 5, 65, ("plain", "symmetric"))]  # (seen: 29, 59)
F_RESTATED = F_CASES[:2]  # the ones small enough for the CPU test to run the restatement on


def big(oracle, case):
    om, Qb, Qs = lattice_graph(oracle, case.dims)
    return Instance(om, Qb, Qs, random_iterate(oracle, Qb.n, om.d, case.r, 5 + case.r))


def big_lambdas(inst, k=1):
    """eigsh(C, which="SA", tol=1e-12) on C itself: t is null, the smallest eigenvalue negative."""
    import scipy.sparse.linalg as spla
    v0 = np.random.default_rng(0).standard_normal(inst.C.shape[0])
    return np.sort(spla.eigsh(inst.C, k=k, which="SA", tol=1e-12, v0=v0, return_eigenvectors=False))


# ---------------------------------------------------------------- H. tiny graphs
H_CASES = [(d, r, n, start) for d in (2, 3) for r in (d, 5) for n in (1, 2, 3, 5) for start in ("random", "truth")]


def tiny(oracle, d, r, n, start):
    """A chain of n poses (n = 1: the first diagonal block of the two-pose chain), at a random X or the noiseless truth."""
    om, Qb, Qs, T = chain_graph(oracle, d, max(n, 2))
    if n == 1:
        b = d + 1
        Qb = oracle.BSR(1, b, np.array([0, 1]), np.array([0]), Qb.vals[:1].copy())
        Qs, T = ref.sparse_Q(Qb), T[:1]
    if start == "random":
        X = random_iterate(oracle, n, d, r, 300 + 10 * n + r)
    else:  # a chain is a tree: composing its measurements gives f = 0
        X = matrix_of(oracle.lift(oracle.odometry_initialization(om, max(n, 2))[:n], r))
    return Instance(om, Qb, Qs, X)
