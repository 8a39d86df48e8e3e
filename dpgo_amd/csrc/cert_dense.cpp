// cert_dense.cpp -- the host algebra of the certificate's eigen-solver (cert_dense.h).  Host compiler only.
#include "cert_dense.h"

#include <algorithm>
#include <cmath>
#include <cstddef>

namespace dpgo_host {
namespace {

constexpr double kJacobiDone = 1e-32;   // jacobi_eig stops when the off-diagonal squares are this share of all squares
constexpr double kRankCut = 1e-10;      // eigenvalues of K K^T at or below this share of the largest are not in K's span
constexpr double kStartShift = 1e-300;  // added to the diagonal of the start block's Gram matrix before its Cholesky
constexpr double kDependent = 1e-7;     // smallest / largest Cholesky pivot of the scaled S S^T below which S is dependent

// The symmetry probe's bound: each entry is an inner product of length L = (d+1) N; its a-priori worst-case rounding
// error is gamma_L |w| |C x| <= L u |W|_F scale' |X|_F with u = 2^-53 and scale' = |C|_2 <= a small multiple of scale (a
// row of C holds the pose's own block and its few neighbours'); the rounding inside the two products C X and C W is of
// the order (row length) u scale |X|_F |W|_F, far below L u for any team.  Two such entries are subtracted, and a
// factor 4 covers scale' / scale: 8 L u, relative to scale |W|_F |X|_F.
double symmetry_bound(int d, int n) { return 8.0 * (double)(d + 1) * (double)n * std::ldexp(1.0, -53); }

}  // namespace

bool cholesky(std::vector<double>& A, int n) {
  for (int j = 0; j < n; ++j) {
    double s = A[j * n + j];
    for (int k = 0; k < j; ++k) s -= A[j * n + k] * A[j * n + k];
    if (!(s > 0.0)) return false;
    const double l = std::sqrt(s);
    A[j * n + j] = l;
    for (int i = j + 1; i < n; ++i) {
      double t = A[i * n + j];
      for (int k = 0; k < j; ++k) t -= A[i * n + k] * A[j * n + k];
      A[i * n + j] = t / l;
    }
    for (int k = j + 1; k < n; ++k) A[j * n + k] = 0.0;
  }
  return true;
}

void jacobi_eig(std::vector<double> A, int n, std::vector<double>& w, std::vector<double>& V) {
  V.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) V[i * n + i] = 1.0;
  for (int sweep = 0; sweep < 100; ++sweep) {
    double off = 0.0, tot = 0.0;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) (i == j ? tot : off) += A[i * n + j] * A[i * n + j];
    if (off <= kJacobiDone * (tot + off) || off == 0.0) break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[p * n + q];
        if (apq == 0.0) continue;
        const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; ++k) {  // A <- A J
          const double akp = A[k * n + p], akq = A[k * n + q];
          A[k * n + p] = c * akp - s * akq;
          A[k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {  // A <- J^T A
          const double apk = A[p * n + k], aqk = A[q * n + k];
          A[p * n + k] = c * apk - s * aqk;
          A[q * n + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < n; ++k) {
          const double vkp = V[k * n + p], vkq = V[k * n + q];
          V[k * n + p] = c * vkp - s * vkq;
          V[k * n + q] = s * vkp + c * vkq;
        }
      }
  }
  std::vector<int> ord(n);
  for (int i = 0; i < n; ++i) ord[i] = i;
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return A[a * n + a] < A[b * n + b]; });
  w.resize(n);
  std::vector<double> Vs((size_t)n * n);
  for (int j = 0; j < n; ++j) {
    w[j] = A[ord[j] * n + ord[j]];
    for (int i = 0; i < n; ++i) Vs[i * n + j] = V[i * n + ord[j]];
  }
  V.swap(Vs);
}

void solve_lt(const std::vector<double>& Lm, int n, std::vector<double>& Y, int m) {
  for (int i = n - 1; i >= 0; --i)
    for (int j = 0; j < m; ++j) {
      double s = Y[i * m + j];
      for (int k = i + 1; k < n; ++k) s -= Lm[k * n + i] * Y[k * m + j];
      Y[i * m + j] = s / Lm[i * n + i];
    }
}

void solve_l_left(const std::vector<double>& Lm, int n, std::vector<double>& A) {
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < n; ++i) {
      double s = A[(size_t)i * n + j];
      for (int k = 0; k < i; ++k) s -= Lm[(size_t)i * n + k] * A[(size_t)k * n + j];
      A[(size_t)i * n + j] = s / Lm[(size_t)i * n + i];
    }
}

void solve_lt_right(const std::vector<double>& Lm, int n, std::vector<double>& A) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      double s = A[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) s -= A[(size_t)i * n + k] * Lm[(size_t)j * n + k];
      A[(size_t)i * n + j] = s / Lm[(size_t)j * n + j];
    }
}

void average_halves(std::vector<double>& A, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < i; ++j) A[(size_t)i * n + j] = A[(size_t)j * n + i] = 0.5 * (A[(size_t)i * n + j] + A[(size_t)j * n + i]);
}

void put_block(std::vector<double>& M, int nb, int r, int k, int j, const std::vector<double>& blk) {
  std::copy(blk.begin(), blk.end(), M.begin() + ((size_t)k * nb + j) * r * r);
}
std::vector<double> eye(int r, double s) {
  std::vector<double> I((size_t)r * r, 0.0);
  for (int a = 0; a < r; ++a) I[a * r + a] = s;
  return I;
}

std::vector<double> assemble_sym(const std::vector<double>& G, int first, int ns, int r) {
  const int m = ns * r;
  std::vector<double> M((size_t)m * m);
  int k = first;
  for (int i = 0; i < ns; ++i)
    for (int j = i; j < ns; ++j, ++k)
      for (int a = 0; a < r; ++a)
        for (int b = 0; b < r; ++b) {  // (i == j: entry (a, b), a > b, is written last by its own turn -- the lower triangle stays)
          const double v = G[(size_t)k * r * r + a * r + b];
          M[(size_t)(i * r + a) * m + j * r + b] = v;
          M[(size_t)(j * r + b) * m + i * r + a] = v;
        }
  return M;
}

DeflationBasis deflation_basis(const std::vector<double>& G, int r, double null_tol) {
  const int m0 = 2 * r;
  const std::vector<double> Gk = assemble_sym(G, 0, 2, r), Gc = assemble_sym(G, 3, 2, r);
  std::vector<double> sk, Uk;
  jacobi_eig(Gk, m0, sk, Uk);
  const double smax = std::max(sk.back(), 0.0);
  std::vector<int> keep;
  for (int i = 0; i < m0; ++i)
    if (sk[i] > kRankCut * smax) keep.push_back(i);
  const int m1 = (int)keep.size();
  // orthonormal basis B^T K of span(K), B = U_keep diag(s^-1/2): m0 x m1
  std::vector<double> Bm((size_t)m0 * m1);
  for (int i = 0; i < m0; ++i)
    for (int j = 0; j < m1; ++j) Bm[(size_t)i * m1 + j] = Uk[(size_t)i * m0 + keep[j]] / std::sqrt(sk[keep[j]]);
  // |C z|^2 on that basis: B^T Gc B, and its near-null eigen-directions
  std::vector<double> H((size_t)m1 * m1, 0.0);
  for (int i = 0; i < m1; ++i)
    for (int j = 0; j < m1; ++j) {
      double s = 0.0;
      for (int a = 0; a < m0; ++a)
        for (int b = 0; b < m0; ++b) s += Bm[(size_t)a * m1 + i] * Gc[(size_t)a * m0 + b] * Bm[(size_t)b * m1 + j];
      H[(size_t)i * m1 + j] = s;
    }
  std::vector<double> mu, Vh;
  if (m1 > 0) jacobi_eig(H, m1, mu, Vh);
  DeflationBasis out;
  for (int i = 0; i < m1; ++i)
    if (std::sqrt(std::max(mu[i], 0.0)) <= null_tol) {
      ++out.mz;
      out.cz = std::max(out.cz, std::sqrt(std::max(mu[i], 0.0)));
    }
  out.mz = std::min(out.mz, 2 * r);
  out.M.assign((size_t)2 * 2 * r * r, 0.0);
  // Z rows = (B V_keep)^T K: coefficient of K row a (block j = a / r) for Z row q (block k = q / r)
  for (int q = 0; q < out.mz; ++q)
    for (int a = 0; a < m0; ++a) {
      double s = 0.0;
      for (int j = 0; j < m1; ++j) s += Bm[(size_t)a * m1 + j] * Vh[(size_t)j * m1 + q];
      const int k = q / r, bq = q % r, jb = a / r, ar = a % r;
      out.M[((size_t)k * 2 + jb) * r * r + ar * r + bq] = s;
    }
  return out;
}

double max_row_norm(const std::vector<double>& Gz, int r, int mz) {
  double v = 0.0;
  for (int q = 0; q < mz; ++q)
    v = std::max(v, std::sqrt(std::max(Gz[(size_t)(q / r) * r * r + (q % r) * r + (q % r)], 0.0)));
  return v;
}

std::vector<double> projection_coefficients(const std::vector<double>& G, int nb, int r) {
  std::vector<double> M((size_t)nb * r * r, 0.0);
  put_block(M, nb, r, 0, 0, eye(r));
  // out row b = v_b - sum_q G[b][q] z_q: coefficient of z_q (row a = q of block j) for output row b is -G[b][a]
  for (int j = 1; j < nb; ++j)
    for (int a = 0; a < r; ++a)
      for (int b = 0; b < r; ++b) M[(size_t)j * r * r + a * r + b] = -G[(size_t)(j - 1) * r * r + b * r + a];
  return M;
}

bool start_block(std::vector<double> G, int r, std::vector<double>& Y) {
  for (int a = 0; a < r; ++a) G[a * r + a] += kStartShift;
  if (!cholesky(G, r)) return false;
  Y = eye(r);
  solve_lt(G, r, Y, r);  // W = L^-1 W2 -> coefficient (row b of W gets sum_a Linv[b][a] w2_a): M[a][b] = Y[a][b]
  return true;
}

std::vector<double> ritz_rotation(std::vector<double> H, int r, std::vector<double>& theta) {
  average_halves(H, r);
  std::vector<double> V;
  jacobi_eig(H, r, theta, V);
  std::vector<double> M((size_t)2 * 2 * r * r, 0.0);
  put_block(M, 2, r, 0, 0, V);
  put_block(M, 2, r, 1, 1, V);
  return M;
}

std::vector<double> residual_coefficients(const std::vector<double>& theta, int r) {
  std::vector<double> M((size_t)2 * r * r, 0.0);
  put_block(M, 2, r, 0, 0, eye(r));
  for (int a = 0; a < r; ++a) M[(size_t)r * r + a * r + a] = -theta[a];
  return M;
}

Ritz rayleigh_ritz(const std::vector<double>& Gr, int ns, int r, std::vector<double>& theta, std::vector<double>& M) {
  const int m = ns * r;
  const std::vector<double> Gs = assemble_sym(Gr, 0, ns, r);
  std::vector<double> Hs = assemble_sym(Gr, ns * (ns + 1) / 2, ns, r);
  average_halves(Hs, m);  // (C symmetric: average the two computed halves of the diagonal blocks)
  // Jacobi scaling, Cholesky of the Gram matrix, the dependence test on its pivots
  std::vector<double> dsc(m);
  for (int i = 0; i < m; ++i) dsc[i] = Gs[(size_t)i * m + i] > 0 ? 1.0 / std::sqrt(Gs[(size_t)i * m + i]) : 0.0;
  std::vector<double> Lm(Gs);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) Lm[(size_t)i * m + j] *= dsc[i] * dsc[j];
  bool okc = cholesky(Lm, m);
  if (okc) {
    double dmin = INFINITY, dmax = 0.0;
    for (int i = 0; i < m; ++i) dmin = std::min(dmin, Lm[(size_t)i * m + i]), dmax = std::max(dmax, Lm[(size_t)i * m + i]);
    okc = dmin > kDependent * dmax;
  }
  if (!okc) return Ritz::dependent;
  // A = L^-1 (D Hs D) L^-T; eigenvectors V; coefficients Y = D L^-T V[:, :r]
  std::vector<double> A((size_t)m * m);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) A[(size_t)i * m + j] = Hs[(size_t)i * m + j] * dsc[i] * dsc[j];
  solve_l_left(Lm, m, A);
  solve_lt_right(Lm, m, A);
  average_halves(A, m);
  std::vector<double> w, V;
  jacobi_eig(A, m, w, V);
  std::vector<double> Y((size_t)m * r);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < r; ++j) Y[(size_t)i * r + j] = V[(size_t)i * m + j];
  solve_lt(Lm, m, Y, r);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < r; ++j) Y[(size_t)i * r + j] *= dsc[i];
  // W' = S Y, P' = [T P] Y_TP, CW' = CS Y, CP' = [CT CP] Y_TP   (inputs W T P CW CT CP)
  const int nb = 2 * ns;
  M.assign((size_t)4 * nb * r * r, 0.0);
  for (int j = 0; j < ns; ++j)
    for (int a = 0; a < r; ++a)
      for (int b = 0; b < r; ++b) {
        const double y = Y[(size_t)(j * r + a) * r + b];
        M[((size_t)0 * nb + j) * r * r + a * r + b] = y;
        M[((size_t)2 * nb + ns + j) * r * r + a * r + b] = y;
        if (j > 0) {
          M[((size_t)1 * nb + j) * r * r + a * r + b] = y;
          M[((size_t)3 * nb + ns + j) * r * r + a * r + b] = y;
        }
      }
  theta.assign(w.begin(), w.begin() + r);
  return Ritz::ok;
}

SymmetryProbe symmetry_probe(const std::vector<double>& G, int r, double scale, int d, int n) {
  double dmax = 0.0, w2 = 0.0, x2 = 0.0;
  for (int e = 0; e < r * r; ++e) dmax = std::max(dmax, std::fabs(G[e] - G[(size_t)r * r + e]));
  for (int a = 0; a < r; ++a) {
    w2 += G[(size_t)2 * r * r + a * r + a];
    x2 += G[(size_t)3 * r * r + a * r + a];
  }
  return {dmax / (scale * std::sqrt(w2) * std::sqrt(x2)), symmetry_bound(d, n)};
}

std::vector<double> normalisation_coefficients(const std::vector<double>& G, int r) {
  std::vector<double> M((size_t)r * r, 0.0);
  for (int a = 0; a < r; ++a) M[a * r + a] = G[a * r + a] > 0 ? 1.0 / std::sqrt(G[a * r + a]) : 0.0;
  return M;
}

}  // namespace dpgo_host
