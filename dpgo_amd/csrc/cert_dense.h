// cert_dense.h -- the host algebra of the certificate's eigen-solver (certify.hip) as plain C++ on
// std::vector<double>: the small dense factorizations, the assembly of a symmetric matrix from Gram blocks, and one pure
// function per step of the solver that turns the r x r Gram blocks the device returned into the coefficient matrix of
// the next per-pose combination.  No HIP, no handle: certify.hip launches, reads Gram blocks back, calls these and
// uploads what they return; tests/cxx/test_cert_dense.cpp calls the unit alone.
//
// Layouts.  Every matrix is row-major.  Gram blocks: r x r each, concatenated in the order of the pass's pair list,
// block k = B[x_k] B[y_k]^T.  Coefficients M: [nout][nb][r][r], out_k = sum_j M[k][j]^T B_j, so M[k][j][a][b] is the
// weight of row a of input block j in row b of output k.
#pragma once
#include <vector>

namespace dpgo_host {

// ---------------------------------------------------------------- small dense linear algebra (row-major n x n)
// Cholesky A = L L^T in place (lower triangle); false if a pivot is not positive
bool cholesky(std::vector<double>& A, int n);
// symmetric eigen-decomposition by cyclic Jacobi: ascending eigenvalues w, eigenvectors in the COLUMNS of V
void jacobi_eig(std::vector<double> A, int n, std::vector<double>& w, std::vector<double>& V);
// X = L^-T Y for lower-triangular L (n x n) and Y (n x m), in place
void solve_lt(const std::vector<double>& Lm, int n, std::vector<double>& Y, int m);
// A <- L^-1 A (forward substitution on columns) and A <- A L^-T, A n x n, in place
void solve_l_left(const std::vector<double>& Lm, int n, std::vector<double>& A);
void solve_lt_right(const std::vector<double>& Lm, int n, std::vector<double>& A);
// A <- (A + A^T) / 2: both halves of every off-diagonal pair get the average
void average_halves(std::vector<double>& A, int n);

// r x r identity / diagonal helpers of the coefficient matrices
void put_block(std::vector<double>& M, int nb, int r, int k, int j, const std::vector<double>& blk);
std::vector<double> eye(int r, double s = 1.0);

// The symmetric (ns r) x (ns r) matrix whose upper-triangle blocks (i, j), i <= j, are the ns (ns + 1) / 2 Gram blocks
// of G from block `first` on, in pair order (0,0) (0,1) .. (0,ns-1) (1,1) ..; block (j, i) is the transpose.  A diagonal
// block is made symmetric from its LOWER triangle (exact for B B^T, whose entries the device sums in one order; for
// W (C W)^T it is the half the solver has always kept).
std::vector<double> assemble_sym(const std::vector<double>& G, int first, int ns, int r);

// ---------------------------------------------------------------- the steps of cert_run, in its order
// Deflation space.  G: blocks of {X, K1, C X, C K1} for the pairs (0,0) (0,1) (1,1) (2,2) (2,3) (3,3), K = [X; K1].
// mz: rows of K's span that one product confirms null (|C z| <= null_tol), at most 2 r; cz: the largest sqrt(mu) among
// them; M [2][2][r][r]: {X, K1} -> {Z0, Z1}, orthonormal rows, rows beyond mz zero (all zero if mz = 0).
struct DeflationBasis {
  int mz = 0;
  double cz = 0.0;
  std::vector<double> M;
  int blocks(int r) const { return (mz + r - 1) / r; }  // Z blocks in use
};
DeflationBasis deflation_basis(const std::vector<double>& G, int r, double null_tol);
// largest row norm among the first mz rows of Z, from the diagonal blocks Gz = {Z0 Z0^T, Z1 Z1^T}
double max_row_norm(const std::vector<double>& Gz, int r, int mz);

// Projection V - sum_j (V B_j^T) B_j onto the complement of nb - 1 orthonormal blocks.  G: V B_j^T, j = 1 .. nb - 1;
// M [1][nb][r][r] for the inputs {V, B_1, ..}
std::vector<double> projection_coefficients(const std::vector<double>& G, int nb, int r);

// Start block.  G = W2 W2^T; Y [1][1][r][r]: {W2} -> {W} orthonormal (W = L^-1 W2).  false: rank deficient
bool start_block(std::vector<double> G, int r, std::vector<double>& Y);

// Ritz rotation of an orthonormal block.  H = W (C W)^T; theta ascending; M [2][2][r][r]: {W, CW} -> {W', CW'}
std::vector<double> ritz_rotation(std::vector<double> H, int r, std::vector<double>& theta);

// Residual block Rs = CW - diag(theta) W.  M [1][2][r][r] for the inputs {CW, W}
std::vector<double> residual_coefficients(const std::vector<double>& theta, int r);

// Rayleigh-Ritz on S = [W, T, P] (ns = 3) or [W, T] (ns = 2).  Gr: the upper-triangle blocks of S S^T, then those of
// S (C S)^T, both in assemble_sym's pair order.  ok: theta = the r smallest Ritz values, M [4][2 ns][r][r]:
// {S.., CS..} -> {W' = S Y, P' = [T P] Y_TP, CW' = CS Y, CP' = [CT CP] Y_TP}.  dependent: the Gram matrix S S^T is
// (near) singular, theta and M untouched -- the caller drops P and repeats, or without P has stagnated.
enum class Ritz { ok, dependent };
Ritz rayleigh_ritz(const std::vector<double>& Gr, int ns, int r, std::vector<double>& theta, std::vector<double>& M);

// Symmetry probe of a team's operator.  G: {W (C X)^T, (C W) X^T, W W^T, X X^T}; L = (d + 1) n is the vectors' length
struct SymmetryProbe {
  double defect, bound;  // max |W (C X)^T - (C W) X^T| relative to scale |W|_F |X|_F, and what rounding alone allows
};
SymmetryProbe symmetry_probe(const std::vector<double>& G, int r, double scale, int d, int n);

// Final normalisation of the reported block's rows.  G = W2 W2^T; M [1][1][r][r]: {W2} -> {W}
std::vector<double> normalisation_coefficients(const std::vector<double>& G, int r);

}  // namespace dpgo_host
