// The host algebra of the certificate's eigen-solver (dpgo_amd/csrc/cert_dense.h / cert_dense.cpp), with the host compiler
// and no library: the small factorizations at every size the solver forms, the block assembly entry by entry, and every
// step's coefficient matrix applied to small explicit matrices (vectors of length N = 12) and compared with what the
// step is defined to produce.  Inputs come from the fixed-seed generator below; no file, no GPU.
#include "cert_dense.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

using namespace dpgo_host;

static int failures = 0;
#define EXPECT(cond)                                                                \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      if (failures < 40) std::printf("cert_dense: line %d: %s\n", __LINE__, #cond); \
      ++failures;                                                                   \
    }                                                                               \
  } while (0)

typedef std::vector<double> Vd;
typedef std::vector<std::pair<int, int>> Pairs;
static const double U = std::ldexp(1.0, -53);
static const int N = 12;  // length of the explicit vectors

struct Rng {
  uint64_t s;
  double next() {  // uniform in [-1, 1)
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(s >> 11) * (2.0 / 9007199254740992.0) - 1.0;
  }
};
static Vd rand_mat(Rng& g, int rows, int cols) {
  Vd A((size_t)rows * cols);
  for (double& v : A) v = g.next();
  return A;
}
static Vd rand_sym(Rng& g, int n) {
  Vd A = rand_mat(g, n, n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < i; ++j) A[i * n + j] = A[j * n + i];
  return A;
}
static double fro(const Vd& A) {
  double s = 0.0;
  for (double v : A) s += v * v;
  return std::sqrt(s);
}
static Vd sub(const Vd& A, const Vd& B) {
  Vd C(A.size());
  for (size_t i = 0; i < A.size(); ++i) C[i] = A[i] - B[i];
  return C;
}
// A (ra x n) times B (rb x n) transposed
static Vd abt(const Vd& A, int ra, const Vd& B, int rb, int n) {
  Vd C((size_t)ra * rb, 0.0);
  for (int i = 0; i < ra; ++i)
    for (int j = 0; j < rb; ++j)
      for (int k = 0; k < n; ++k) C[i * rb + j] += A[i * n + k] * B[j * n + k];
  return C;
}
// A (m x k) times B (k x n)
static Vd ab(const Vd& A, int m, const Vd& B, int k, int n) {
  Vd C((size_t)m * n, 0.0);
  for (int i = 0; i < m; ++i)
    for (int l = 0; l < k; ++l)
      for (int j = 0; j < n; ++j) C[i * n + j] += A[i * k + l] * B[l * n + j];
  return C;
}
static Vd identity(int n) {
  Vd I((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) I[i * n + i] = 1.0;
  return I;
}
// the device's Gram pass: block k = B[x_k] B[y_k]^T (r x r), concatenated
static Vd grams(const std::vector<Vd>& B, const Pairs& pairs, int r) {
  Vd G;
  for (const auto& p : pairs) {
    const Vd g = abt(B[p.first], r, B[p.second], r, N);
    G.insert(G.end(), g.begin(), g.end());
  }
  return G;
}
// the device's combination pass: out_k = sum_j M[k][j]^T B_j, M [nout][nb][r][r]
static std::vector<Vd> combine(const std::vector<Vd>& B, const Vd& M, int nout, int r) {
  const int nb = (int)B.size();
  EXPECT(M.size() == (size_t)nout * nb * r * r);
  std::vector<Vd> out(nout, Vd((size_t)r * N, 0.0));
  if (M.size() != (size_t)nout * nb * r * r) return out;
  for (int k = 0; k < nout; ++k)
    for (int j = 0; j < nb; ++j)
      for (int a = 0; a < r; ++a)
        for (int b = 0; b < r; ++b)
          for (int c = 0; c < N; ++c) out[k][b * N + c] += M[((size_t)k * nb + j) * r * r + a * r + b] * B[j][a * N + c];
  return out;
}
// rows of A (rows x n) made orthonormal in place by Gram-Schmidt (two passes); a row whose remainder is below tol of the
// longest row is zeroed.  Returns the number of rows kept: the rank
static int gram_schmidt(Vd& A, int rows, int n, double tol) {
  int rank = 0;
  double len0 = 0.0;
  for (int i = 0; i < rows; ++i) {
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += A[i * n + k] * A[i * n + k];
    len0 = std::max(len0, s);
  }
  for (int i = 0; i < rows; ++i) {
    for (int pass = 0; pass < 2; ++pass)
      for (int j = 0; j < i; ++j) {
        double s = 0.0;
        for (int k = 0; k < n; ++k) s += A[i * n + k] * A[j * n + k];
        for (int k = 0; k < n; ++k) A[i * n + k] -= s * A[j * n + k];
      }
    double len = 0.0;
    for (int k = 0; k < n; ++k) len += A[i * n + k] * A[i * n + k];
    const bool keep = std::sqrt(len) > tol * std::sqrt(len0);
    for (int k = 0; k < n; ++k) A[i * n + k] = keep ? A[i * n + k] / std::sqrt(len) : 0.0;
    rank += keep;
  }
  return rank;
}
static Vd stack(const std::vector<Vd>& B) {
  Vd S;
  for (const Vd& b : B) S.insert(S.end(), b.begin(), b.end());
  return S;
}
static Vd rows_of(const Vd& A, int first, int count) { return Vd(A.begin() + (size_t)first * N, A.begin() + (size_t)(first + count) * N); }

// ---------------------------------------------------------------- jacobi_eig, cholesky, solve_lt and the two sweeps
// Every bound is a multiple of n u |A|_F (u = 2^-53).  The multiples in the comments were measured on these inputs with the
// code as it stood in certify.hip; each bound allows four times that for the compiler's freedom.  The loosest, 24 n u at
// n = 15, is 4e-14.
static double worst_eig = 0.0, worst_orth = 0.0, worst_chol = 0.0, worst_solve = 0.0, worst_sweep = 0.0;

static void check_eig(const Vd& A, int n) {
  Vd w, V;
  jacobi_eig(A, n, w, V);
  EXPECT((int)w.size() == n && (int)V.size() == n * n);
  for (int i = 0; i + 1 < n; ++i) EXPECT(w[i] <= w[i + 1]);
  Vd VD(V);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) VD[i * n + j] *= w[j];
  const double unit = n * U * std::max(fro(A), 1e-300);
  const double res = fro(sub(ab(A, n, V, n, n), VD)) / unit;
  Vd Vt(V);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) Vt[i * n + j] = V[j * n + i];
  const double orth = fro(sub(abt(Vt, n, Vt, n, n), identity(n))) / (n * U);
  worst_eig = std::max(worst_eig, res);
  worst_orth = std::max(worst_orth, orth);
  EXPECT(res <= 6.1);    // |A V - V diag(w)|_F: measured 1.51 n u |A|_F, allowed 6.1
  EXPECT(orth <= 24.0);  // |V^T V - I|_F:        measured 5.77 n u,        allowed 24
}

static void test_dense() {
  Rng g{11};
  for (int n : {1, 2, 3, 6, 9, 15}) {
    check_eig(rand_sym(g, n), n);
    Vd D((size_t)n * n, 0.0);  // diagonal, descending: no rotation, only the sort
    for (int i = 0; i < n; ++i) D[i * n + i] = (double)(n - i) + 0.25 * g.next();
    check_eig(D, n);
    Vd R = identity(n);  // I + x x^T: eigenvalue 1 repeated n - 1 times
    const Vd x = rand_mat(g, 1, n);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) R[i * n + j] += x[i] * x[j];
    check_eig(R, n);
    {
      Vd w, V;
      jacobi_eig(R, n, w, V);
      for (int i = 0; i + 1 < n; ++i) EXPECT(std::fabs(w[i] - 1.0) <= 24.0 * n * U * fro(R));
    }

    // Cholesky of B B^T + n I, then the three triangular solves against it
    const Vd B = rand_mat(g, n, n);
    Vd A = abt(B, n, B, n, n);
    for (int i = 0; i < n; ++i) A[i * n + i] += n;
    Vd L(A);
    EXPECT(cholesky(L, n));
    for (int i = 0; i < n; ++i)
      for (int j = i + 1; j < n; ++j) EXPECT(L[i * n + j] == 0.0);
    const double chol = fro(sub(abt(L, n, L, n, n), A)) / (n * U * fro(A));
    worst_chol = std::max(worst_chol, chol);
    EXPECT(chol <= 5.9);  // |L L^T - A|_F: measured 1.47 n u |A|_F, allowed 5.9
    Vd Lt(L);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) Lt[i * n + j] = L[j * n + i];
    for (int m : {1, n}) {  // X = L^-T Y
      const Vd Y = rand_mat(g, n, m);
      Vd X(Y);
      solve_lt(L, n, X, m);
      const double e = fro(sub(ab(Lt, n, X, n, m), Y)) / (n * U * fro(L) * fro(X));
      worst_solve = std::max(worst_solve, e);
      EXPECT(e <= 5.1);  // |L^T X - Y|_F: measured 1.26 n u |L|_F |X|_F, allowed 5.1
    }
    const Vd Y = rand_mat(g, n, n);
    Vd X1(Y), X2(Y);
    solve_l_left(L, n, X1);    // X1 = L^-1 Y
    solve_lt_right(L, n, X2);  // X2 = Y L^-T
    const double e1 = fro(sub(ab(L, n, X1, n, n), Y)) / (n * U * fro(L) * fro(X1));
    const double e2 = fro(sub(ab(X2, n, Lt, n, n), Y)) / (n * U * fro(L) * fro(X2));
    worst_sweep = std::max(worst_sweep, std::max(e1, e2));
    EXPECT(e1 <= 0.72 && e2 <= 0.72);  // |L X1 - Y|_F, |X2 L^T - Y|_F: measured 0.18 n u |L|_F |X|_F, allowed 0.72
  }
  // a pivot that is not positive
  Vd zero_pivot{1.0, 1.0, 1.0, 1.0}, negative_pivot{1.0, 2.0, 2.0, 1.0}, z1{0.0}, n1{-1.0};
  EXPECT(!cholesky(zero_pivot, 2));
  EXPECT(!cholesky(negative_pivot, 2));
  EXPECT(!cholesky(z1, 1));
  EXPECT(!cholesky(n1, 1));
  Vd S{1.0, 2.0, 3.0, 4.0};
  average_halves(S, 2);
  EXPECT(S[0] == 1.0 && S[1] == 2.5 && S[2] == 2.5 && S[3] == 4.0);
}

// ---------------------------------------------------------------- assemble_sym, put_block, eye
static void test_assembly() {
  for (int ns : {2, 3})
    for (int r : {2, 5})
      for (int first : {0, 2}) {
        const int np = ns * (ns + 1) / 2, m = ns * r;
        auto enc = [](int k, int a, int b) { return 1000.0 * k + 10.0 * a + b; };
        Vd G((size_t)(first + np) * r * r, -1.0);  // (blocks before `first` must not be read)
        for (int k = 0; k < np; ++k)
          for (int a = 0; a < r; ++a)
            for (int b = 0; b < r; ++b) G[(size_t)(first + k) * r * r + a * r + b] = enc(k, a, b);
        const Vd M = assemble_sym(G, first, ns, r);
        EXPECT((int)M.size() == m * m);
        int k = 0;
        for (int i = 0; i < ns; ++i)
          for (int j = i; j < ns; ++j, ++k)
            for (int a = 0; a < r; ++a)
              for (int b = 0; b < r; ++b) {
                if (i == j) {  // the lower triangle of a diagonal block, mirrored
                  EXPECT(M[(size_t)(i * r + a) * m + i * r + b] == enc(k, std::max(a, b), std::min(a, b)));
                } else {
                  EXPECT(M[(size_t)(i * r + a) * m + j * r + b] == enc(k, a, b));
                  EXPECT(M[(size_t)(j * r + b) * m + i * r + a] == enc(k, a, b));
                }
              }
      }
  const Vd I = eye(3, 2.0);
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) EXPECT(I[a * 3 + b] == (a == b ? 2.0 : 0.0));
  Vd M((size_t)2 * 3 * 4, 0.0);  // [nout = 2][nb = 3][2][2]
  put_block(M, 3, 2, 1, 2, Vd{1.0, 2.0, 3.0, 4.0});
  for (size_t e = 0; e < M.size(); ++e) EXPECT(M[e] == (e >= 20 ? (double)(e - 19) : 0.0));
}

// ---------------------------------------------------------------- deflation basis
// C = sum_{i >= 4} lambda_i q_i q_i^T on R^12 with lambda in [1, 2]: null space span(q_0 .. q_3), |C|_2 <= 2.  K = [X; t]
// (2 r rows, t in row 0 of the second block, the rest zero as on the device).  The null directions inside span(K) number
// rank(K) - rank(K C), both ranks by Gram-Schmidt in the test.
static void check_deflation(const Vd& C, const Vd& X, const Vd& K1, int r, int expect_mz) {
  const std::vector<Vd> B{X, K1, ab(X, r, C, N, N), ab(K1, r, C, N, N)};
  const Vd G = grams(B, {{0, 0}, {0, 1}, {1, 1}, {2, 2}, {2, 3}, {3, 3}}, r);
  const double null_tol = 1e-6 * 2.0;
  const DeflationBasis D = deflation_basis(G, r, null_tol);
  Vd K = stack({X, K1}), CK = stack({B[2], B[3]});
  const Vd K0(K);
  const int rank_k = gram_schmidt(K, 2 * r, N, 1e-8), rank_ck = gram_schmidt(CK, 2 * r, N, 1e-8);
  EXPECT(D.mz == rank_k - rank_ck);
  EXPECT(D.mz == expect_mz);
  EXPECT(D.blocks(r) == (D.mz + r - 1) / r);
  EXPECT(D.cz <= null_tol);
  const std::vector<Vd> Zb = combine({X, K1}, D.M, 2, r);
  const Vd Z = stack(Zb), ZZ = abt(Z, 2 * r, Z, 2 * r, N), CZ = ab(Z, 2 * r, C, N, N);
  // Orthonormal rows: the kept eigenvalues of K K^T are within 1e3 of each other on these inputs, so the basis carries a
  // few hundred u; C Z is null to sqrt(u) |C| |K| at worst (mu is an eigenvalue of a Gram matrix of squares).
  for (int p = 0; p < 2 * r; ++p) {
    for (int q = 0; q < 2 * r; ++q) EXPECT(std::fabs(ZZ[p * 2 * r + q] - (p == q && p < D.mz ? 1.0 : 0.0)) <= 1e-12);
    if (p >= D.mz)
      for (int c = 0; c < N; ++c) EXPECT(Z[p * N + c] == 0.0);
    EXPECT(fro(rows_of(CZ, p, 1)) <= null_tol);
  }
  // span: every row of K that C annihilates is reproduced by its projection on Z
  for (int a = 0; a < 2 * r; ++a) {
    const Vd k = rows_of(K0, a, 1);
    if (fro(k) == 0.0 || fro(ab(k, 1, C, N, N)) > 1e-12) continue;
    Vd rem(k);
    for (int q = 0; q < D.mz; ++q) {
      double s = 0.0;
      for (int c = 0; c < N; ++c) s += k[c] * Z[q * N + c];
      for (int c = 0; c < N; ++c) rem[c] -= s * Z[q * N + c];
    }
    EXPECT(fro(rem) <= 1e-10 * fro(k));
  }
}

static void test_deflation() {
  Rng g{23};
  Vd Q = rand_mat(g, N, N);
  EXPECT(gram_schmidt(Q, N, N, 1e-8) == N);
  Vd C((size_t)N * N, 0.0);
  for (int i = 4; i < N; ++i) {
    const double lam = 1.5 + 0.5 * g.next();
    for (int a = 0; a < N; ++a)
      for (int b = 0; b < N; ++b) C[a * N + b] += lam * Q[i * N + a] * Q[i * N + b];
  }
  auto null_vec = [&]() {  // a random vector of span(q_0 .. q_3)
    Vd v(N, 0.0);
    for (int i = 0; i < 4; ++i) {
      const double w = g.next();
      for (int c = 0; c < N; ++c) v[c] += w * Q[i * N + c];
    }
    return v;
  };
  auto set_row = [](Vd& A, int row, const Vd& v) { std::copy(v.begin(), v.end(), A.begin() + (size_t)row * N); };
  for (int r : {3, 5}) {
    // full rank: every row of X null but the last, t null -> r null directions among r + 1
    Vd X = rand_mat(g, r, N), K1((size_t)r * N, 0.0);
    for (int a = 0; a + 1 < std::min(r, 4); ++a) set_row(X, a, null_vec());
    set_row(K1, 0, null_vec());
    const int nulls = std::min(r, 4) - 1;  // null rows of X (the null space has 4 dimensions: t takes the last)
    check_deflation(C, X, K1, r, nulls + 1);
    // two equal rows of X: the rank cut drops one direction, the null count loses it too
    Vd X2(X);
    set_row(X2, 1, rows_of(X2, 0, 1));
    check_deflation(C, X2, K1, r, nulls);
    // t inside the row space of X
    Vd K2((size_t)r * N, 0.0), t(N);
    for (int c = 0; c < N; ++c) t[c] = X[c] + 0.5 * X[N + c];
    set_row(K2, 0, t);
    check_deflation(C, X, K2, r, nulls);
    // nothing null: no Z block, M all zero
    const Vd Xn = rand_mat(g, r, N);
    Vd Kn((size_t)r * N, 0.0);
    set_row(Kn, 0, rand_mat(g, 1, N));
    check_deflation(C, Xn, Kn, r, 0);
  }
  // the reported residual: the largest row norm among the first mz rows of Z
  const Vd Gz{4.0, 9.0, 9.0, 16.0, /**/ 25.0, 0.0, 0.0, 100.0};
  EXPECT(max_row_norm(Gz, 2, 0) == 0.0 && max_row_norm(Gz, 2, 1) == 2.0 && max_row_norm(Gz, 2, 2) == 4.0);
  EXPECT(max_row_norm(Gz, 2, 3) == 5.0 && max_row_norm(Gz, 2, 4) == 10.0);
}

// ---------------------------------------------------------------- projection, start block, Ritz rotation, residual, normalisation
static void test_coefficients() {
  Rng g{37};
  for (int r : {2, 5}) {
    const Vd C = rand_sym(g, N);
    // out_b = v_b - sum_j sum_q G_j[b][q] z_{j,q}
    for (int nb : {2, 3}) {
      std::vector<Vd> B;
      for (int j = 0; j < nb; ++j) B.push_back(rand_mat(g, r, N));
      Pairs pairs;
      for (int j = 1; j < nb; ++j) pairs.push_back({0, j});
      const Vd G = grams(B, pairs, r);
      const Vd out = combine(B, projection_coefficients(G, nb, r), 1, r)[0];
      Vd want(B[0]);
      for (int j = 1; j < nb; ++j)
        for (int b = 0; b < r; ++b)
          for (int q = 0; q < r; ++q)
            for (int c = 0; c < N; ++c) want[b * N + c] -= G[(size_t)(j - 1) * r * r + b * r + q] * B[j][q * N + c];
      EXPECT(fro(sub(out, want)) <= 8.0 * N * U * fro(want));  // (the same sums in another order)
    }
    // start block: W = L^-1 W2 is orthonormal, row b a combination of rows a <= b of W2
    const Vd W2 = rand_mat(g, r, N);
    Vd Y;
    EXPECT(start_block(abt(W2, r, W2, r, N), r, Y));
    for (int a = 0; a < r; ++a)
      for (int b = 0; b < a; ++b) EXPECT(Y[a * r + b] == 0.0);
    const Vd W = combine({W2}, Y, 1, r)[0];
    // (|W W^T - I| <= u cond(W2 W2^T) times a small factor; r random rows of length 12 keep cond below 1e3)
    EXPECT(fro(sub(abt(W, r, W, r, N), identity(r))) <= 1e-12);
    Vd dup((size_t)r * N, 0.0);  // two equal rows of squared length 4: the second pivot is exactly 0
    for (int c = 0; c < 4; ++c) dup[c] = dup[N + c] = 1.0;
    for (int a = 2; a < r; ++a) dup[a * N + 4 + a] = 1.0;
    Vd Yd{-7.0};
    EXPECT(!start_block(abt(dup, r, dup, r, N), r, Yd));
    // Ritz rotation: {W, CW} -> {W', CW'}, W' C W'^T = diag(theta) ascending, W' orthonormal, CW' = W' C
    const Vd CW = ab(W, r, C, N, N);
    Vd theta;
    const std::vector<Vd> rot = combine({W, CW}, ritz_rotation(abt(W, r, CW, r, N), r, theta), 2, r);
    EXPECT((int)theta.size() == r);
    for (int a = 0; a + 1 < r; ++a) EXPECT(theta[a] <= theta[a + 1]);
    EXPECT(fro(sub(abt(rot[0], r, rot[0], r, N), identity(r))) <= 1e-12);
    EXPECT(fro(sub(rot[1], ab(rot[0], r, C, N, N))) <= 1e-12 * fro(C));
    Vd Dt((size_t)r * r, 0.0);
    for (int a = 0; a < r; ++a) Dt[a * r + a] = theta[a];
    EXPECT(fro(sub(abt(rot[0], r, rot[1], r, N), Dt)) <= 1e-12 * fro(C));
    // residual: Rs = CW - diag(theta) W, inputs {CW, W}
    const Vd Rs = combine({rot[1], rot[0]}, residual_coefficients(theta, r), 1, r)[0];
    for (int a = 0; a < r; ++a)
      for (int c = 0; c < N; ++c) {
        const double cw = rot[1][a * N + c], tw = theta[a] * rot[0][a * N + c];
        EXPECT(std::fabs(Rs[a * N + c] - (cw - tw)) <= 2.0 * U * (std::fabs(cw) + std::fabs(tw)));
      }
    // normalisation: unit rows; a zero row stays zero
    Vd V = rand_mat(g, r, N);
    for (int c = 0; c < N; ++c) V[(r - 1) * N + c] = 0.0;
    const Vd Vn = combine({V}, normalisation_coefficients(abt(V, r, V, r, N), r), 1, r)[0];
    for (int a = 0; a < r; ++a) {
      EXPECT(std::fabs(fro(rows_of(Vn, a, 1)) - (a + 1 < r ? 1.0 : 0.0)) <= 8.0 * U);
      for (int c = 0; c < N; ++c) EXPECT(std::fabs(Vn[a * N + c] * fro(rows_of(V, a, 1)) - V[a * N + c]) <= 8.0 * U);
    }
  }
}

// ---------------------------------------------------------------- Rayleigh-Ritz step
static Vd ritz_grams(const std::vector<Vd>& S, const Vd& C, int ns, int r, std::vector<Vd>* all) {
  std::vector<Vd> B(S.begin(), S.begin() + ns);
  for (int j = 0; j < ns; ++j) B.push_back(ab(S[j], r, C, N, N));
  Pairs pairs;
  for (int i = 0; i < ns; ++i)
    for (int j = i; j < ns; ++j) pairs.push_back({i, j});
  for (int i = 0; i < ns; ++i)
    for (int j = i; j < ns; ++j) pairs.push_back({i, ns + j});
  if (all) *all = B;
  return grams(B, pairs, r);
}

static void test_rayleigh_ritz() {
  Rng g{41};
  for (int r : {2, 3})  // (3 r = 9 rows fit into R^12)
    for (int ns : {2, 3}) {
      const int m = ns * r, nb = 2 * ns;
      const Vd C = rand_sym(g, N);
      Vd W = rand_mat(g, r, N);
      EXPECT(gram_schmidt(W, r, N, 1e-8) == r);
      const std::vector<Vd> S{W, rand_mat(g, r, N), rand_mat(g, r, N)};
      std::vector<Vd> B;
      const Vd Gr = ritz_grams(S, C, ns, r, &B);
      Vd theta(r, -7.0), M;
      EXPECT(rayleigh_ritz(Gr, ns, r, theta, M) == Ritz::ok);
      // the pencil (S C S^T, S S^T) on an orthonormal basis of span(S); Gram-Schmidt pivots above 0.05 keep
      // cond(S S^T) below 1e4, and both routes carry u cond m |C|: 1e-10 |C|_F leaves two orders
      Vd Qs = stack(std::vector<Vd>(S.begin(), S.begin() + ns));
      EXPECT(gram_schmidt(Qs, m, N, 0.05) == m);
      Vd A = abt(ab(Qs, m, C, N, N), m, Qs, m, N);
      average_halves(A, m);
      Vd w, V;
      jacobi_eig(A, m, w, V);
      EXPECT((int)theta.size() == r);
      for (int a = 0; a < r && a < (int)theta.size(); ++a) EXPECT(std::fabs(theta[a] - w[a]) <= 1e-10 * fro(C));
      const std::vector<Vd> out = combine(B, M, 4, r);  // W', P', CW', CP'
      EXPECT(fro(sub(abt(out[0], r, out[0], r, N), identity(r))) <= 1e-10);
      EXPECT(fro(sub(out[2], ab(out[0], r, C, N, N))) <= 1e-10 * fro(C));
      EXPECT(fro(sub(out[3], ab(out[1], r, C, N, N))) <= 1e-10 * fro(C));
      // P' is W' without its W part; W' and P' read no C S block, CW' and CP' no S block
      const Vd Yw(M.begin(), M.begin() + r * r);
      const Vd Wpart = combine({W}, Yw, 1, r)[0];
      EXPECT(fro(sub(out[1], sub(out[0], Wpart))) <= 16.0 * U * fro(out[0]));
      for (int k = 0; k < 4; ++k)
        for (int j = 0; j < nb; ++j) {
          const bool used = (k < 2 ? j < ns : j >= ns) && !(k % 2 == 1 && j % ns == 0);
          const double* blk = &M[((size_t)k * nb + j) * r * r];
          const double* src = &M[((size_t)0 * nb + j % ns) * r * r];
          for (int e = 0; e < r * r; ++e) EXPECT(blk[e] == (used ? src[e] : 0.0));
        }
      if (ns < 3) continue;
      // P with a row equal to a row of W to 1e-9: dependent, nothing written; without P the step goes through
      std::vector<Vd> Sp(S);
      for (int c = 0; c < N; ++c) Sp[2][c] = W[c] + 1e-9 * g.next();
      Vd theta2(r, -7.0), M2{-7.0};
      EXPECT(rayleigh_ritz(ritz_grams(Sp, C, 3, r, nullptr), 3, r, theta2, M2) == Ritz::dependent);
      EXPECT(theta2 == Vd(r, -7.0) && M2 == Vd{-7.0});
      EXPECT(rayleigh_ritz(ritz_grams(Sp, C, 2, r, nullptr), 2, r, theta2, M2) == Ritz::ok);
      // T with such a row: dependent with P, and dependent again once the caller has dropped P -- its stagnation exit
      std::vector<Vd> St(S);
      for (int c = 0; c < N; ++c) St[1][c] = W[c] + 1e-9 * g.next();
      Vd theta3(r, -7.0), M3{-7.0};
      EXPECT(rayleigh_ritz(ritz_grams(St, C, 3, r, nullptr), 3, r, theta3, M3) == Ritz::dependent);
      EXPECT(rayleigh_ritz(ritz_grams(St, C, 2, r, nullptr), 2, r, theta3, M3) == Ritz::dependent);
      EXPECT(theta3 == Vd(r, -7.0) && M3 == Vd{-7.0});
      // The threshold itself.  A perturbation of 1e-9 is below what a Gram matrix in doubles can see (sqrt(u) = 1e-8), so
      // the two cases above hold for any threshold.  Here P's row leaves W's along a unit vector orthogonal to all of S:
      // the smallest pivot of the scaled Gram matrix is eps (to 1e-8), the largest 1 -- dependent below 1e-7, not above.
      Vd Qn = stack(S);
      const Vd extra = rand_mat(g, 1, N);
      Qn.insert(Qn.end(), extra.begin(), extra.end());
      EXPECT(gram_schmidt(Qn, m + 1, N, 0.05) == m + 1);
      for (double eps : {4e-8, 1e-6}) {
        for (int c = 0; c < N; ++c) Sp[2][c] = W[c] + eps * Qn[m * N + c];
        EXPECT(rayleigh_ritz(ritz_grams(Sp, C, 3, r, nullptr), 3, r, theta2, M2) == (eps < 1e-7 ? Ritz::dependent : Ritz::ok));
      }
    }
}

// ---------------------------------------------------------------- symmetry defect and its bound
static void test_symmetry() {
  const int r = 2;
  // {W (C X)^T, (C W) X^T, W W^T, X X^T}: |W|_F^2 = 4, |X|_F^2 = 9
  Vd G{1.0, -2.0, 3.0, 0.5, /**/ 1.0, -2.0, 3.0, 0.5, /**/ 1.0, 7.0, 7.0, 3.0, /**/ 4.0, -1.0, -1.0, 5.0};
  SymmetryProbe s = symmetry_probe(G, r, 2.0, 3, 100);
  EXPECT(s.defect == 0.0);
  EXPECT(s.bound == 8.0 * 4.0 * 100.0 * std::ldexp(1.0, -53));
  G[6] += 0.5;
  s = symmetry_probe(G, r, 2.0, 2, 7);
  EXPECT(s.defect == 0.5 / (2.0 * 2.0 * 3.0));
  EXPECT(s.bound == 8.0 * 3.0 * 7.0 * std::ldexp(1.0, -53));
}

int main() {
  test_dense();
  test_assembly();
  test_deflation();
  test_coefficients();
  test_rayleigh_ritz();
  test_symmetry();
  if (failures) {
    std::printf("cert_dense: %d failures\n", failures);
    return 1;
  }
  std::printf("cert_dense: ok (n u multiples: eig %.2f orth %.2f chol %.2f solve %.2f sweeps %.2f)\n", worst_eig, worst_orth,
              worst_chol, worst_solve, worst_sweep);
  return 0;
}
