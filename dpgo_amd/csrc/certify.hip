// certify.hip -- certificate of global optimality of a rank-r iterate (SE-Sync / DC2-PGO verification) and the
// Riemannian-staircase escape along its witness.  DESIGN.md section 10.
//
// C(X) = Q - Lambda(X), Lambda = blockdiag(Lambda_i), Lambda_i = [sym(Y_i^T (XQ)_rot,i) 0; 0 0].  The smallest eigenvalue of
// C on the complement of the known null space Z (rows of X, translation indicator) is found by a preconditioned block
// LOBPCG whose block is one r-row tile vector (the handle's compiled (d, r) instance): products with C, Gram blocks and
// per-pose linear combinations run on the device (kernels/certify.h); only the r x r Gram blocks and the coefficient
// matrices of the 3r x 3r Rayleigh-Ritz problem cross PCIe.
#include "host.h"

namespace dpgo_host {
namespace {

// ---------------------------------------------------------------- the solver's device state
// CW = W C(X) (k_cert_apply) on `g` workgroups: the symmetric copy of Q at one pose per d+1 lanes, or Q at the handle's split
int launch_cert_apply(dpgo_problem_s* p, int d, int r, bool sym, int g, const double* S, const double* W, double* CW,
                      double* part, int n) {
  CHK(dispatch_drs(d, r, p->split, [&](auto D, auto R, auto SPLIT) {
    if (sym) return launch(k_cert_apply<D, R, 1, BsrSymDev>, g, 0, p->stream, p->sym.dev(), S, W, CW, part, n);
    return launch(k_cert_apply<D, R, SPLIT>, g, 0, p->stream, p->Q.dev(), S, W, CW, part, n);
  }));
  HIPC(hipGetLastError());
  return DPGO_OK;
}

// A team of agents side by side on one device and stream (include/dpgo_hip.h, dpgo_team_certify_device): the handles, the
// slice of the team vector each owns, the device tables of k_cert_apply_team.  With a team, Cert's pose vectors hold
// N = sum n_a tiles, `apply` is one launch over the tile table and `precondition` goes member by member on its slice;
// Gram blocks, combinations and the Rayleigh-Ritz code never know.
struct Team {
  std::vector<dpgo_problem_s*> h;
  std::vector<int> first, precond;
  int N = 0, ntiles = 0;
  std::vector<DevBuf<int32_t>> nbr;  // nbr_pose of every member (device)
  DevBuf<int32_t> no_rows;           // an all-zero rowptr: the coupling of a member without neighbours
  DevBuf<CertMember> members;
  DevBuf<CertTile> tiles;
  DevBuf<double> tin, tout;          // 16-byte-aligned staging of a slice the multilevel cycle cannot take in place
};
// workgroups of a launch over the team's tile table: at most the first member's DPGO_GRID_HESS cap (second trips can be
// forced as for k_cert_apply)
int team_grid(const Team& t) { return std::max(1, std::min(t.ntiles, t.h[0]->cap_h)); }

struct Cert {
  dpgo_problem_s* p;  // (a team: its first member -- the stream, the device, the launch cap)
  Team* team = nullptr;
  int d, r, n;
  bool sym = false;     // products read the symmetric copy of Q
  DevBuf<double> S;     // Lambda blocks at X (k_grad)
  DevBuf<double> zero;  // a zero iterate: the multilevel cycle's projection at it is the identity
  DevBuf<double> part;  // per-workgroup partials
  DevBuf<double> red;   // reduced Gram blocks (device)
  DevBuf<double> coef;  // coefficient matrices of k_cert_combine (device)
  DevBuf<double> qdiag; // per-workgroup maxima of q_scale
  PinBuf<double> hbuf;  // reduced Gram blocks (host)
  PinBuf<double> hcoef; // coefficient ring
  std::vector<DevBuf<double>> vecs;  // the solver's pose vectors (vec)
  int coef_slot = 0;
  int products = 0;
  int precond = DPGO_PRECOND_NONE;
  double shift = 0.1;
  static constexpr int kCoefSlots = 8;
  static constexpr int kCoefCap = kCertMaxOut * kCertMaxBlocks * 36;
  static constexpr int kGramWg = 512;  // workgroups of k_cert_gram (partials: kGramWg x kCertMaxPairs x 36)

  explicit Cert(dpgo_problem_s* h) : p(h), d(h->d), r(h->r), n(h->n) {}
  explicit Cert(Team& t) : p(t.h[0]), team(&t), d(p->d), r(p->r), n(t.N) {}

  size_t vec_bytes() const { return (size_t)n * (d + 1) * r * sizeof(double); }
  int flat_grid() const {
    const size_t cols = (size_t)n * (d + 1);
    return (int)std::max<size_t>(1, std::min<size_t>(kMaxGrid, (cols + kBlock - 1) / kBlock));
  }
  int vec(double** out) {
    vecs.emplace_back();
    CHK(vecs.back().alloc((size_t)n * (d + 1) * r));
    *out = vecs.back();
    return DPGO_OK;
  }
  int init() {
    CHK(S.alloc((size_t)n * d * d));
    CHK(part.alloc((size_t)std::max(kPartialCap * 36, kGramWg * kCertMaxPairs * 36)));
    CHK(red.alloc(kCertMaxPairs * 36));
    CHK(coef.alloc(kCoefSlots * kCoefCap));
    CHK(hbuf.alloc(kCertMaxPairs * 36));
    CHK(hcoef.alloc(kCoefSlots * kCoefCap));
    return DPGO_OK;
  }

  // CW = W C(X); with wcw != null also W CW^T (r x r, row-major) on the host
  int apply(const double* W, double* CW, std::vector<double>* wcw = nullptr) {
    const int g = team ? team_grid(*team) : sym ? p->grid_outer_sym() : p->grid_s();  // (a team: one launch)
    if (team) {
      CHK(dispatch_dr(d, r, [&](auto D, auto R) {
        return launch(k_cert_apply_team<D, R>, g, 0, p->stream, team->members, team->tiles, team->ntiles, W, CW, part);
      }));
      HIPC(hipGetLastError());
    } else {
      CHK(launch_cert_apply(p, d, r, sym, g, S, W, CW, part, n));
    }
    ++products;
    if (wcw) CHK(reduce(g, r * r, *wcw));
    return DPGO_OK;
  }
  int reduce(int nwg, int E, std::vector<double>& out) {
    launch(k_cert_reduce, (E + kBlock - 1) / kBlock, 0, p->stream, part, nwg, E, red);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(hbuf, red, sizeof(double) * E, hipMemcpyDeviceToHost, p->stream));
    HIPC(hipStreamSynchronize(p->stream));
    out.assign(hbuf.get(), hbuf + E);
    return DPGO_OK;
  }
  // G[k] = B[x_k] B[y_k]^T for every pair k (r x r blocks, row-major, concatenated)
  int gram(const std::vector<const double*>& B, const std::vector<std::pair<int, int>>& pairs, std::vector<double>& G) {
    if (B.size() > (size_t)kCertMaxBlocks || pairs.size() > (size_t)kCertMaxPairs || pairs.empty())
      return fail(DPGO_ERR_INVALID, "certify: Gram pass too large");
    CertIn in{};
    CertPairs pr{};
    for (size_t j = 0; j < B.size(); ++j) in.b[j] = B[j];
    for (size_t k = 0; k < pairs.size(); ++k) {
      pr.x[k] = (int8_t)pairs[k].first;
      pr.y[k] = (int8_t)pairs[k].second;
    }
    const size_t chunks = ((size_t)n * (d + 1) + kCertCols - 1) / kCertCols;
    const int g = (int)std::max<size_t>(1, std::min<size_t>(kGramWg, chunks));
    const int nb = (int)B.size(), np = (int)pairs.size();
    CHK(dispatch_dr(d, r, [&](auto D, auto R) {
      return launch(k_cert_gram<D, R, kCertMaxBlocks>, g, 0, p->stream, in, nb, pr, np, part, n);
    }));
    HIPC(hipGetLastError());
    return reduce(g, np * r * r, G);
  }
  // out_k = sum_j M[k][j]^T B_j; M: [nout][nb][r][r] row-major
  int combine(const std::vector<const double*>& B, const std::vector<double*>& out, const std::vector<double>& M) {
    if (B.size() > (size_t)kCertMaxBlocks || out.size() > (size_t)kCertMaxOut ||
        M.size() != out.size() * B.size() * r * r)
      return fail(DPGO_ERR_INVALID, "certify: combination too large");
    CertIn in{};
    CertOut o{};
    for (size_t j = 0; j < B.size(); ++j) in.b[j] = B[j];
    for (size_t k = 0; k < out.size(); ++k) o.b[k] = out[k];
    double* h = hcoef + (size_t)coef_slot * kCoefCap;
    double* dv = coef + (size_t)coef_slot * kCoefCap;
    coef_slot = (coef_slot + 1) % kCoefSlots;  // (the stream is synchronised by every Gram read-back, several per ring turn)
    std::copy(M.begin(), M.end(), h);
    HIPC(hipMemcpyAsync(dv, h, sizeof(double) * M.size(), hipMemcpyHostToDevice, p->stream));
    const int nb = (int)B.size(), nout = (int)out.size();
    CHK(dispatch_dr(d, r, [&](auto D, auto R) {
      return launch(k_cert_combine<D, R, kCertMaxBlocks>, flat_grid(), 0, p->stream, in, nb, o, nout, (const double*)dv, n);
    }));
    HIPC(hipGetLastError());
    return DPGO_OK;
  }
  // Z = M^-1 V without tangent projection
  int precondition(const double* V, double* Z) {
    if (team) {  // block diagonal over the members: each one's factors or cycle on its own slice
      for (size_t a = 0; a < team->h.size(); ++a) {
        dpgo_problem_s* q = team->h[a];
        const size_t o = (size_t)team->first[a] * q->T;
        const double* Vs = V + o;
        double* Zs = Z + o;
        if (team->precond[a] == DPGO_PRECOND_BLOCK_JACOBI) {
          CHK(dispatch_dr(d, r, [&](auto D, auto R) {
            return launch(k_cert_jacobi<D, R>, q->grid(), 0, q->stream, Vs, q->dinv, Zs, q->n);
          }));
          HIPC(hipGetLastError());
        } else if (team->precond[a] == DPGO_PRECOND_MULTILEVEL) {
          if (aligned16(Vs) && aligned16(Zs)) {
            CHK(launch_ml_apply(q, zero, Vs, Zs));
          } else {  // (odd tile sizes: a slice starts on an 8-byte boundary, the cycle moves 16-byte pieces)
            HIPC(hipMemcpyAsync(team->tin, Vs, q->vec_bytes(), hipMemcpyDeviceToDevice, q->stream));
            CHK(launch_ml_apply(q, zero, team->tin, team->tout));
            HIPC(hipMemcpyAsync(Zs, team->tout, q->vec_bytes(), hipMemcpyDeviceToDevice, q->stream));
          }
        } else {
          HIPC(hipMemcpyAsync(Zs, Vs, q->vec_bytes(), hipMemcpyDeviceToDevice, q->stream));
        }
      }
      return DPGO_OK;
    }
    if (precond == DPGO_PRECOND_BLOCK_JACOBI) {
      CHK(dispatch_dr(d, r, [&](auto D, auto R) {
        return launch(k_cert_jacobi<D, R>, p->grid(), 0, p->stream, V, p->dinv, Z, n);
      }));
      HIPC(hipGetLastError());
    } else if (precond == DPGO_PRECOND_MULTILEVEL) {
      CHK(launch_ml_apply(p, zero, V, Z));
    } else {
      HIPC(hipMemcpyAsync(Z, V, vec_bytes(), hipMemcpyDeviceToDevice, p->stream));
    }
    return DPGO_OK;
  }
};

// max_i max diag(Q_ii)
int q_scale(dpgo_problem_s* p, DevBuf<double>& dv, double* out) {
  const int g = (p->n + kBlock - 1) / kBlock;
  CHK(dv.alloc(g));
  if (p->d == 2)
    launch(k_cert_scale<2>, g, 0, p->stream, p->Q.dev(), dv, p->n);
  else
    launch(k_cert_scale<3>, g, 0, p->stream, p->Q.dev(), dv, p->n);
  HIPC(hipGetLastError());
  std::vector<double> h(g);
  HIPC(hipMemcpyAsync(h.data(), dv, sizeof(double) * g, hipMemcpyDeviceToHost, p->stream));
  HIPC(hipStreamSynchronize(p->stream));
  double m = 0.0;
  for (double v : h) m = std::max(m, v);
  *out = m;
  return DPGO_OK;
}

int resolve_params(const dpgo_certify_params* prm_in, dpgo_certify_params& prm) {
  if (prm_in)
    prm = *prm_in;
  else
    dpgo_certify_params_default(&prm);
  if (!(prm.eta >= 0.0) || !(prm.tol_rel > 0.0) || prm.max_iterations < 1 || !(prm.precond_shift >= 0.0))
    return fail(DPGO_ERR_INVALID, "certify: bad parameters");
  return DPGO_OK;
}
// what the handle's AUTO / ADDITIVE mean for the certificate's preconditioner
int resolve_precond(dpgo_problem_s* p, int precond, int* out) {
  if (precond == DPGO_PRECOND_AUTO) {
    p->auto_decide();
    precond = p->auto_ml ? DPGO_PRECOND_MULTILEVEL : DPGO_PRECOND_BLOCK_JACOBI;
  }
  if (precond == DPGO_PRECOND_ADDITIVE) precond = DPGO_PRECOND_MULTILEVEL;  // (the additive form lives inside the one-launch solve only)
  if (precond < DPGO_PRECOND_NONE || precond > DPGO_PRECOND_MULTILEVEL) return fail(DPGO_ERR_INVALID, "unknown preconditioner");
  *out = precond;
  return DPGO_OK;
}

int cert_run(Cert& c, const double* X, const dpgo_certify_params& prm, double scale, dpgo_certify_result* res,
             double* witness, bool witness_on_host, std::chrono::steady_clock::time_point t0, double* symmetry_defect);

int certify_impl(dpgo_problem_s* p, const double* X, const dpgo_certify_params* prm_in, dpgo_certify_result* res,
                 double* witness, bool witness_on_host) {
  const auto t0 = std::chrono::steady_clock::now();
  CHK(check_ready(p));
  if (!X || !res) return fail(DPGO_ERR_INVALID, "null pointer");
  if (p->has_G || p->C.nnzb > 0)
    return fail(DPGO_ERR_INVALID, "certification is defined for a problem without a linear term G (global / central problem)");
  dpgo_certify_params prm;
  CHK(resolve_params(prm_in, prm));
  int precond = 0;
  CHK(resolve_precond(p, prm.precond, &precond));
  *res = dpgo_certify_result{};
  res->status = DPGO_CERT_NOT_CONVERGED;

  Cert c(p);
  c.precond = precond;
  c.shift = prm.precond_shift;
  CHK(c.init());
  if (p->sym_wanted() && p->split == 1) {
    bool usable = false;
    CHK(sym_ensure(p, &usable));
    c.sym = usable;
  }
  // Lambda at X (and f, |rgrad| on the way)
  CHK(eval_state(p, X, c.S, c.sym));
  res->gradnorm = p->hstate->ngf;
  double scale = 0.0;
  CHK(q_scale(p, c.qdiag, &scale));
  if (!(scale > 0.0)) return fail(DPGO_ERR_INVALID, "certify: Q has no positive diagonal");
  if (precond == DPGO_PRECOND_BLOCK_JACOBI) CHK(build_dinv(p, prm.precond_shift));
  if (precond == DPGO_PRECOND_MULTILEVEL) {
    CHK(ml_ensure(p, prm.precond_shift));
    CHK(ml_ops32_ensure(p));
    CHK(c.zero.alloc((size_t)c.n * (c.d + 1) * c.r));
    HIPC(hipMemsetAsync(c.zero, 0, c.vec_bytes(), p->stream));
  }
  return cert_run(c, X, prm, scale, res, witness, witness_on_host, t0, nullptr);
}

// The eigen-solver on Cert's operator, one handle or a team alike.  symmetry_defect (a team): the probe of the operator's
// symmetry from the two products the solver makes anyway (below).
// This function is the device side: vectors, launches, Gram read-backs, loop control.  Every coefficient matrix it hands to
// Cert::combine, and every decision taken from a Gram block, comes from cert_dense.h.
int cert_run(Cert& c, const double* X, const dpgo_certify_params& prm, double scale, dpgo_certify_result* res,
             double* witness, bool witness_on_host, std::chrono::steady_clock::time_point t0, double* symmetry_defect) {
  dpgo_problem_s* p = c.p;
  const int r = c.r;
  res->scale = scale;
  const double eta = prm.eta * scale, tol = prm.tol_rel * scale;
  const double null_tol = std::sqrt(prm.tol_rel) * scale;  // a candidate direction z is null when |C z| <= this

  // ---- deflation space: rows of X and the translation indicator, kept where one product confirms them null
  double *K1, *CK0, *CK1, *Z0, *Z1;
  for (double** v : {&K1, &CK0, &CK1, &Z0, &Z1}) CHK(c.vec(v));
  CHK(dispatch_dr(c.d, r, [&](auto D, auto R) {
    return launch(k_cert_indicator<D, R>, c.flat_grid(), 0, p->stream, K1, c.n);
  }));
  HIPC(hipGetLastError());
  CHK(c.apply(X, CK0));
  CHK(c.apply(K1, CK1));
  std::vector<double> G;
  CHK(c.gram({X, K1, CK0, CK1}, {{0, 0}, {0, 1}, {1, 1}, {2, 2}, {2, 3}, {3, 3}}, G));
  const DeflationBasis defl = deflation_basis(G, r, null_tol);
  res->deflated = defl.mz;
  res->deflation_residual = defl.cz;
  const int nzb = defl.blocks(r);  // Z blocks (rows beyond mz are zero)
  // the reported |C z| (in place on CK0, CK1: a team's symmetry probe reads C X first, so there it runs behind the probe)
  auto deflation_residual = [&]() -> int {
    if (nzb == 0) return DPGO_OK;
    // mu is an eigenvalue of a Gram matrix of squares, so sqrt(mu) carries sqrt(round-off) of the
    // LARGEST |C k| (1e-8 of it: an exactly null t beside a non-stationary X reads 1e-11 scale).  C Z is the same
    // combination of C K, and its row norms have no such cancellation.
    CHK(c.combine({CK0, CK1}, {CK0, CK1}, defl.M));
    std::vector<double> Gz;
    CHK(c.gram({CK0, CK1}, {{0, 0}, {1, 1}}, Gz));
    res->deflation_residual = max_row_norm(Gz, r, defl.mz);
    return DPGO_OK;
  };
  if (nzb > 0) {
    CHK(c.combine({X, K1}, {Z0, Z1}, defl.M));
    if (!symmetry_defect) CHK(deflation_residual());
  }
  std::vector<const double*> Zb;
  if (nzb >= 1) Zb.push_back(Z0);
  if (nzb >= 2) Zb.push_back(Z1);

  // ---- block LOBPCG on the complement of Z
  double *W, *T, *P, *CW, *CT, *CP, *W2, *P2, *CW2, *CP2, *Rs;
  for (double** v : {&W, &T, &P, &CW, &CT, &CP, &W2, &P2, &CW2, &CP2, &Rs}) CHK(c.vec(v));
  CHK(dispatch_dr(c.d, r, [&](auto D, auto R) {
    return launch(k_cert_random<D, R>, c.flat_grid(), 0, p->stream, (unsigned long long)prm.seed, W, c.n);
  }));
  HIPC(hipGetLastError());
  // V <- V - (V Z^T) Z - (V U^T) U for orthonormal Z blocks and (optionally) an orthonormal block U; into `out`
  auto project = [&](const double* V, const double* U, double* out) -> int {
    std::vector<const double*> B{V};
    std::vector<std::pair<int, int>> pairs;
    for (const double* z : Zb) {
      pairs.push_back({0, (int)B.size()});
      B.push_back(z);
    }
    if (U) {
      pairs.push_back({0, (int)B.size()});
      B.push_back(U);
    }
    if (pairs.empty()) {
      if (out != V) HIPC(hipMemcpyAsync(out, V, c.vec_bytes(), hipMemcpyDeviceToDevice, p->stream));
      return DPGO_OK;
    }
    std::vector<double> Gp;
    CHK(c.gram(B, pairs, Gp));
    return c.combine(B, {out}, projection_coefficients(Gp, (int)B.size(), r));
  };
  // W <- Ritz vectors of W (orthonormalised against itself, rotated to diagonalise W C W^T); theta ascending
  std::vector<double> theta(r, 0.0), M;
  CHK(project(W, nullptr, W2));
  CHK(c.gram({W2}, {{0, 0}}, G));
  if (!start_block(G, r, M)) return fail(DPGO_ERR_STATE, "certify: start block is rank deficient");
  CHK(c.combine({W2}, {W}, M));
  CHK(c.apply(W, CW));
  CHK(c.gram({W, CW}, {{0, 1}}, G));
  CHK(c.combine({W, CW}, {W2, CW2}, ritz_rotation(G, r, theta)));
  std::swap(W, W2);
  std::swap(CW, CW2);
  if (symmetry_defect) {
    // A team's pieces form a symmetric operator only if both owners of every shared edge hold the same weight and
    // activity for it.  The start block W and the iterate X have both been multiplied by now (CW above, CK0 = C X of the
    // deflation step): for a symmetric C the r x r blocks W (C X)^T and (C W) X^T are equal up to rounding
    // (symmetry_probe's bound).
    CHK(c.gram({W, CK0, CW, X}, {{0, 1}, {2, 3}, {0, 0}, {3, 3}}, G));
    const SymmetryProbe probe = symmetry_probe(G, r, scale, c.d, c.n);
    *symmetry_defect = probe.defect;
    if (!(probe.defect <= probe.bound))
      return fail(DPGO_ERR_STATE, "team certificate: agents hold different weights or activity for a shared edge "
                                  "(symmetry defect " + std::to_string(probe.defect) + " of scale)");
    CHK(deflation_residual());
  }
  bool have_p = false, negative = false;
  double resid0 = 0.0;
  int it = 0;
  for (; it < prm.max_iterations; ++it) {
    // residual block Rs = CW - diag(theta) W and its row norms
    CHK(c.combine({CW, W}, {Rs}, residual_coefficients(theta, r)));
    CHK(c.gram({Rs}, {{0, 0}}, G));
    resid0 = std::sqrt(std::max(G[0], 0.0));
    if (theta[0] < -eta) negative = true;
    if (resid0 <= tol) break;
    // T = M^-1 Rs, orthogonal to Z and W
    CHK(c.precondition(Rs, T));
    CHK(project(T, W, T));
    CHK(c.apply(T, CT));
    // Rayleigh-Ritz on S = [W, T, P]: the upper-triangle blocks of S S^T, then of S (C S)^T
    const int ns = have_p ? 3 : 2;
    std::vector<const double*> Sb{W, T, P}, CSb{CW, CT, CP};
    std::vector<const double*> B;
    std::vector<std::pair<int, int>> pairs;
    for (int j = 0; j < ns; ++j) B.push_back(Sb[j]);
    for (int j = 0; j < ns; ++j) B.push_back(CSb[j]);
    for (int i = 0; i < ns; ++i)
      for (int j = i; j < ns; ++j) pairs.push_back({i, j});
    for (int i = 0; i < ns; ++i)
      for (int j = i; j < ns; ++j) pairs.push_back({i, ns + j});
    CHK(c.gram(B, pairs, G));
    // a (near) dependent P is dropped and the step repeated without it
    if (rayleigh_ritz(G, ns, r, theta, M) == Ritz::dependent) {
      if (have_p) {
        have_p = false;
        --it;
        continue;
      }
      break;  // T depends on W: the iteration has stagnated
    }
    CHK(c.combine(B, {W2, P2, CW2, CP2}, M));
    std::swap(W, W2);
    std::swap(P, P2);
    std::swap(CW, CW2);
    std::swap(CP, CP2);
    have_p = true;
  }
  const bool converged = resid0 <= tol;
  if (theta[0] < -eta) negative = true;
  // the reported pair: the first Ritz vector, projected onto the complement of Z once more, normalised, and its exact
  // Rayleigh quotient
  CHK(project(W, nullptr, W2));
  CHK(c.gram({W2}, {{0, 0}}, G));
  CHK(c.combine({W2}, {W}, normalisation_coefficients(G, r)));
  std::vector<double> wcw;
  CHK(c.apply(W, CW, &wcw));
  res->lambda_min = wcw[0];
  res->residual = resid0;
  res->iterations = it;
  res->products = c.products;
  if (res->lambda_min < -eta || negative)
    res->status = DPGO_CERT_NOT_CERTIFIED;
  else if (converged)
    res->status = DPGO_CERT_CERTIFIED;
  else
    res->status = DPGO_CERT_NOT_CONVERGED;
  if (witness) {
    const size_t ncol = (size_t)c.n * (c.d + 1);
    HIPC(hipMemcpy2DAsync(witness, sizeof(double), W, sizeof(double) * r, sizeof(double), ncol,
                          witness_on_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, p->stream));
  }
  HIPC(hipStreamSynchronize(p->stream));
  res->elapsedMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return DPGO_OK;
}

// ---------------------------------------------------------------- a team of agents (include/dpgo_hip.h)
// Checks of the member table that need no device, then the device, then the handles: nothing is dereferenced before it
// is known to be a handle of this process's device.
int team_check(const dpgo_team_member* mem, int n_members, Team& t) {
  if (!mem || n_members < 1) return fail(DPGO_ERR_INVALID, "team: no members");
  for (int a = 0; a < n_members; ++a) {
    if (!mem[a].h) return fail(DPGO_ERR_INVALID, "team: null handle");
    if (mem[a].first < 0 || (a == 0 && mem[a].first != 0) || (a > 0 && mem[a].first <= mem[a - 1].first))
      return fail(DPGO_ERR_INVALID, "team: the members' slices do not tile [0, N) in member order");
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    (void)hipGetLastError();
    return fail(DPGO_ERR_HIP, "team: no HIP device");
  }
  dpgo_problem_s* p0 = mem[0].h;
  int N = 0;
  for (int a = 0; a < n_members; ++a) {
    dpgo_problem_s* q = mem[a].h;
    if (!q->Q.vals) return fail(DPGO_ERR_STATE, "team: quadratic matrix Q not set");
    if (q->pending.active) return fail(DPGO_ERR_STATE, "team: a member has a solve in flight");
    if (q->d != p0->d || q->r != p0->r) return fail(DPGO_ERR_INVALID, "team: members differ in (d, r)");
    if (q->device != p0->device || q->stream != p0->stream)
      return fail(DPGO_ERR_INVALID, "team: members on different devices or streams");
    if (q->g0_nonzero) return fail(DPGO_ERR_INVALID, "team: a member has priors (a constant term in G): out of scope");
    if (mem[a].first != N) return fail(DPGO_ERR_INVALID, "team: the members' slices do not tile [0, N) in member order");
    if ((long long)N + q->n > 0x7fffffffLL) return fail(DPGO_ERR_INVALID, "team: too many poses");
    N += q->n;
  }
  for (int a = 0; a < n_members; ++a) {
    dpgo_problem_s* q = mem[a].h;
    const int nc = q->C.rowptr ? q->C.ncols : 0;
    if (nc > 0 && !mem[a].nbr_pose) return fail(DPGO_ERR_INVALID, "team: null nbr_pose");
    for (int k = 0; k < nc; ++k) {
      const int j = mem[a].nbr_pose[k];
      if (j < 0 || j >= N || (j >= mem[a].first && j < mem[a].first + q->n))
        return fail(DPGO_ERR_INVALID, "team: nbr_pose entry outside [0, N) or inside the member's own slice");
    }
    t.h.push_back(q);
    t.first.push_back(mem[a].first);
  }
  t.N = N;
  return DPGO_OK;
}

// device tables of the team kernels (k_cert_apply_team, k_team_eval): members, tiles, every member's nbr_pose.  S: the team's
// Lambda blocks [N, d, d] the member table points into, or null for a kernel that reads none
int team_tables(const dpgo_team_member* mem, Team& t, double* S) {
  dpgo_problem_s* p0 = t.h[0];
  CHK(set_device(p0));
  const int d = p0->d, P = (64 / (d + 1)) * kWaves, na = (int)t.h.size();
  int nmax = 0;
  for (dpgo_problem_s* q : t.h) nmax = std::max(nmax, q->n);
  CHK(t.no_rows.alloc((size_t)nmax + 1));
  HIPC(hipMemsetAsync(t.no_rows, 0, sizeof(int32_t) * ((size_t)nmax + 1), p0->stream));
  std::vector<CertMember> hm(na);
  std::vector<CertTile> ht;
  t.nbr.resize(na);
  for (int a = 0; a < na; ++a) {
    dpgo_problem_s* q = t.h[a];
    const int nc = q->C.rowptr ? q->C.ncols : 0;
    CHK(upload(t.nbr[a], mem[a].nbr_pose, (size_t)nc, q->stream));
    hm[a].Q = q->Q.dev();
    hm[a].C = q->C.rowptr ? q->C.dev() : BsrDev{t.no_rows, nullptr, nullptr};
    hm[a].nbr_pose = t.nbr[a];
    hm[a].S = S ? S + (size_t)t.first[a] * d * d : nullptr;
    hm[a].first = t.first[a];
    hm[a].n = q->n;
    for (int p0_ = 0; p0_ < q->n; p0_ += P) ht.push_back(CertTile{a, p0_});
  }
  t.ntiles = (int)ht.size();
  CHK(upload(t.members, hm.data(), hm.size(), p0->stream));
  CHK(upload(t.tiles, ht.data(), ht.size(), p0->stream));
  HIPC(hipStreamSynchronize(p0->stream));  // (the tables are host vectors of this scope, nbr_pose the caller's)
  return DPGO_OK;
}

// the tables, every G_a from the team's X (the member's linear term as an exchange of X would leave it), every member's
// S, f and |rgrad| (S: the team's Lambda blocks, [N, d, d]); gn2 = sum |rgrad_a|^2 in member order
int team_setup(const dpgo_team_member* mem, Team& t, const double* X, double* S, double* gn2) {
  CHK(team_tables(mem, t, S));
  const int d = t.h[0]->d, T = t.h[0]->T;
  int cmax = 0;
  for (dpgo_problem_s* q : t.h) cmax = std::max(cmax, q->C.rowptr ? q->C.ncols : 0);
  DevBuf<double> nbuf;  // neighbour tiles of one member at a time
  CHK(nbuf.alloc((size_t)std::max(cmax, 1) * T));
  double sum = 0.0;
  for (size_t a = 0; a < t.h.size(); ++a) {
    dpgo_problem_s* q = t.h[a];
    const int nc = q->C.rowptr ? q->C.ncols : 0;
    if (q->C.rowptr) {
      if (nc > 0) {
        launch(k_cert_gather_tiles, flat_grid((size_t)nc * T), 0, q->stream, X, t.nbr[a], T, nc, nbuf);
        HIPC(hipGetLastError());
      }
      CHK(refresh_G(q, nbuf));
    }
    CHK(eval_state(q, X + (size_t)t.first[a] * T, S + (size_t)t.first[a] * d * d));  // (synchronises: nbuf is free again)
    sum += q->hstate->ngf * q->hstate->ngf;
  }
  *gn2 = sum;
  return DPGO_OK;
}

// f and |rgrad f| of a team's iterate, one launch and the reduce (k_team_eval): what an escape trial and the sweep loop's
// stopping test need, without the members' G
struct TeamEval {
  DevBuf<double> part, red;
  PinBuf<double> host;
  int init() {
    CHK(part.alloc((size_t)kPartialCap * 2));
    CHK(red.alloc(2));
    CHK(host.alloc(2));
    return DPGO_OK;
  }
  // rank r of the compiled (d, r) instance is the caller's: the tables hold nothing that depends on it
  int run(const Team& t, int d, int r, const double* X, double* RG, double* f, double* gn) {
    dpgo_problem_s* p0 = t.h[0];
    const int g = team_grid(t);
    CHK(dispatch_dr(d, r, [&](auto Dc, auto Rc) {
      constexpr int D = decltype(Dc)::value, R = decltype(Rc)::value;
      auto go = [&](auto kernel) {
        return launch(kernel, g, 0, p0->stream, t.members, t.tiles, t.ntiles, X, RG, part);
      };
      return RG ? go(k_team_eval<D, R, true>) : go(k_team_eval<D, R, false>);
    }));
    launch(k_cert_reduce, 1, 0, p0->stream, part, g, 2, red);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(host, red, sizeof(double) * 2, hipMemcpyDeviceToHost, p0->stream));
    HIPC(hipStreamSynchronize(p0->stream));
    *f = 0.5 * host[0];
    *gn = std::sqrt(host[1]);
    return DPGO_OK;
  }
};

int team_certify_impl(const dpgo_team_member* mem, int n_members, const double* X, const dpgo_certify_params* prm_in,
                      dpgo_team_certify_result* out, double* witness) {
  const auto t0 = std::chrono::steady_clock::now();
  if (!X || !out) return fail(DPGO_ERR_INVALID, "null pointer");
  dpgo_certify_params prm;
  CHK(resolve_params(prm_in, prm));
  Team t;
  CHK(team_check(mem, n_members, t));
  *out = dpgo_team_certify_result{};
  out->cert.status = DPGO_CERT_NOT_CONVERGED;
  out->members = n_members;
  out->poses = t.N;
  dpgo_problem_s* p0 = t.h[0];
  Cert c(t);
  c.shift = prm.precond_shift;
  CHK(set_device(p0));
  CHK(c.init());
  double gn2 = 0.0, scale = 0.0;
  CHK(team_setup(mem, t, X, c.S, &gn2));
  out->cert.gradnorm = std::sqrt(gn2);
  int nml = 0;
  bool staged = false;
  for (size_t a = 0; a < t.h.size(); ++a) {
    dpgo_problem_s* q = t.h[a];
    double sa = 0.0;
    CHK(q_scale(q, c.qdiag, &sa));
    scale = std::max(scale, sa);
    int pc = 0;
    CHK(resolve_precond(q, prm.precond, &pc));
    t.precond.push_back(pc);
    if (pc == DPGO_PRECOND_BLOCK_JACOBI) CHK(build_dinv(q, prm.precond_shift));
    if (pc == DPGO_PRECOND_MULTILEVEL) {
      CHK(ml_ensure(q, prm.precond_shift));
      CHK(ml_ops32_ensure(q));
      nml = std::max(nml, q->n);
      staged = staged || (((size_t)t.first[a] * q->T) & 1);
    }
  }
  if (!(scale > 0.0)) return fail(DPGO_ERR_INVALID, "certify: Q has no positive diagonal");
  if (nml > 0) {
    CHK(c.zero.alloc((size_t)nml * p0->T));
    HIPC(hipMemsetAsync(c.zero, 0, sizeof(double) * (size_t)nml * p0->T, p0->stream));
    if (staged) {
      CHK(t.tin.alloc((size_t)nml * p0->T));
      CHK(t.tout.alloc((size_t)nml * p0->T));
    }
  }
  return cert_run(c, X, prm, scale, &out->cert, witness, false, t0, &out->symmetry_defect);
}

// The staircase's step along a witness over n poses.  SE-Sync's rule: the first of alpha0, alpha0 / 2, ... whose retraction
// decreases f below f0 and leaves the gradient above the tolerance (the next solve must not stop at once); alpha0 moves
// each pose by ~0.1 for a witness spread over all poses.  trial(alpha, &f, &gn) makes the step and evaluates it.
// alpha, trials: the accepted step (0 if none) and the trials made, either may be null
template <class Trial>
int halving_search(int n, double f0, double grad_tol, Trial trial, double* alpha, int* trials) {
  double a = 0.1 * std::sqrt((double)n);
  for (int k = 0; k < 60; ++k, a *= 0.5) {
    double f = 0.0, gn = 0.0;
    CHK(trial(a, &f, &gn));
    if (trials) *trials = k + 1;
    if (f < f0 && gn > grad_tol) {
      if (alpha) *alpha = a;
      return DPGO_OK;
    }
  }
  if (alpha) *alpha = 0.0;
  return fail(DPGO_ERR_STATE, "certify: no step along the witness decreases f");
}

}  // namespace
}  // namespace dpgo_host

extern "C" {

void dpgo_certify_params_default(dpgo_certify_params* p) {
  if (!p) return;
  p->eta = 1e-6;
  p->tol_rel = 1e-6;
  p->max_iterations = 1000;
  p->precond = DPGO_PRECOND_AUTO;
  p->precond_shift = 1e-1;
  p->seed = 1;
}


int dpgo_problem_certify_device(dpgo_problem_t h, const double* X_dev, const dpgo_certify_params* params,
                                dpgo_certify_result* result, double* witness_dev) {
  return certify_impl(h, X_dev, params, result, witness_dev, false);
}


int dpgo_problem_certify(dpgo_problem_t h, const double* X_host, const dpgo_certify_params* params,
                         dpgo_certify_result* result, double* witness_host) {
  CHK(check_ready(h));
  if (!X_host) return fail(DPGO_ERR_INVALID, "null X");
  DevBuf<double> X;
  CHK(X.alloc((size_t)h->n * h->T));
  CHK(h2d(h, X, X_host));
  return certify_impl(h, X, params, result, witness_host, true);
}


int dpgo_problem_certificate_apply(dpgo_problem_t h, const double* X_host, const double* V_host, double* CV_host) {
  CHK(check_ready(h));
  if (!X_host || !V_host || !CV_host) return fail(DPGO_ERR_INVALID, "null pointer");
  if (h->has_G || h->C.nnzb > 0)
    return fail(DPGO_ERR_INVALID, "the certificate matrix is defined for a problem without a linear term G");
  DevBuf<double> X, V, CV, S, part;
  for (DevBuf<double>* v : {&X, &V, &CV}) CHK(v->alloc((size_t)h->n * h->T));
  CHK(S.alloc((size_t)h->n * h->d * h->d));
  CHK(part.alloc((size_t)kPartialCap * 36));
  CHK(h2d(h, X, X_host));
  CHK(h2d(h, V, V_host));
  bool sym = false;
  if (h->sym_wanted() && h->split == 1) CHK(sym_ensure(h, &sym));
  CHK(launch_grad(h, X, nullptr, S, nullptr, nullptr, sym));
  CHK(launch_cert_apply(h, h->d, h->r, sym, sym ? h->grid_outer_sym() : h->grid_s(), S, V, CV, part, h->n));
  return d2h(h, CV_host, CV);
}


int dpgo_team_certify_device(const dpgo_team_member* members, int n_members, const double* X_team_dev,
                             const dpgo_certify_params* params, dpgo_team_certify_result* result,
                             double* witness_team_dev) {
  if (!aligned8(X_team_dev) || !aligned8(witness_team_dev)) return fail(DPGO_ERR_INVALID, "team: pointer not 8-byte aligned");
  return team_certify_impl(members, n_members, X_team_dev, params, result, witness_team_dev);
}


int dpgo_team_certificate_apply_gram_device(const dpgo_team_member* members, int n_members, const double* X_team_dev,
                                            const double* V_team_dev, double* CV_team_dev, double* vcv_host) {
  if (!X_team_dev || !V_team_dev || !CV_team_dev) return fail(DPGO_ERR_INVALID, "null pointer");
  if (!aligned8(X_team_dev) || !aligned8(V_team_dev) || !aligned8(CV_team_dev))
    return fail(DPGO_ERR_INVALID, "team: pointer not 8-byte aligned");
  Team t;
  CHK(team_check(members, n_members, t));
  dpgo_problem_s* p0 = t.h[0];
  CHK(set_device(p0));
  Cert c(t);
  CHK(c.S.alloc((size_t)t.N * p0->d * p0->d));
  CHK(c.part.alloc((size_t)kPartialCap * 36));
  double gn2 = 0.0;
  CHK(team_setup(members, t, X_team_dev, c.S, &gn2));
  if (vcv_host) {
    CHK(c.red.alloc(36));
    CHK(c.hbuf.alloc(36));
    std::vector<double> vcv;
    CHK(c.apply(V_team_dev, CV_team_dev, &vcv));
    std::copy(vcv.begin(), vcv.end(), vcv_host);
  } else {
    CHK(c.apply(V_team_dev, CV_team_dev));
  }
  HIPC(hipStreamSynchronize(p0->stream));
  return DPGO_OK;
}


int dpgo_team_certificate_apply_device(const dpgo_team_member* members, int n_members, const double* X_team_dev,
                                       const double* V_team_dev, double* CV_team_dev) {
  return dpgo_team_certificate_apply_gram_device(members, n_members, X_team_dev, V_team_dev, CV_team_dev, nullptr);
}


int dpgo_certify_escape_device(dpgo_problem_t h_next, int r, const double* X_dev, const double* witness_dev,
                               double grad_tol, double* X_next_dev, double* alpha) {
  if (!h_next) return fail(DPGO_ERR_INVALID, "null handle");
  if (!supported(h_next->d, r + 1)) return fail(DPGO_ERR_UNSUPPORTED, "certify: (d, r + 1) not compiled in");
  if (h_next->r != r + 1) return fail(DPGO_ERR_INVALID, "certify: the escape handle must have rank r + 1");
  if (!X_dev || !witness_dev || !X_next_dev) return fail(DPGO_ERR_INVALID, "null pointer");
  if (!(grad_tol >= 0.0)) return fail(DPGO_ERR_INVALID, "certify: bad gradient tolerance");
  CHK(check_ready(h_next));
  dpgo_problem_s* p = h_next;
  const int g = std::max(1, std::min(kMaxGrid, (int)(((size_t)p->n * (p->d + 1) + kBlock - 1) / kBlock)));
  DevBuf<double> Xl;
  CHK(Xl.alloc((size_t)p->n * p->T));
  auto lift = [&](double a) -> int {
    CHK(dispatch_dr(p->d, r, [&](auto D, auto R) {
      return launch(k_cert_lift<D, R>, g, 0, p->stream, X_dev, witness_dev, a, Xl, p->n);
    }));
    HIPC(hipGetLastError());
    return DPGO_OK;
  };
  double f0 = 0.0, gn0 = 0.0;
  CHK(lift(0.0));
  CHK(dpgo_problem_eval_device(p, Xl, &f0, &gn0));
  auto trial = [&](double a, double* f, double* gn) -> int {
    CHK(lift(a));
    CHK(launch_retract(p, Xl, Xl, 0.0, X_next_dev, nullptr));
    return dpgo_problem_eval_device(p, X_next_dev, f, gn);
  };
  return halving_search(p->n, f0, grad_tol, trial, alpha, nullptr);
}


int dpgo_team_eval_device(const dpgo_team_member* members, int n_members, const double* X_team_dev, double* f,
                          double* gradnorm, double* rgrad_team_dev) {
  if (!X_team_dev || !f || !gradnorm) return fail(DPGO_ERR_INVALID, "null pointer");
  if (!aligned8(X_team_dev) || !aligned8(rgrad_team_dev)) return fail(DPGO_ERR_INVALID, "team: pointer not 8-byte aligned");
  Team t;
  CHK(team_check(members, n_members, t));
  CHK(team_tables(members, t, nullptr));
  TeamEval ev;
  CHK(ev.init());
  return ev.run(t, t.h[0]->d, t.h[0]->r, X_team_dev, rgrad_team_dev, f, gradnorm);
}


int dpgo_team_escape_device(const dpgo_team_member* members_next, int n_members, int r, const double* X_team_dev,
                            const double* witness_team_dev, double grad_tol, double* X_next_team_dev,
                            dpgo_team_escape_result* out) {
  if (!X_team_dev || !witness_team_dev || !X_next_team_dev || !out) return fail(DPGO_ERR_INVALID, "null pointer");
  if (!aligned8(X_team_dev) || !aligned8(witness_team_dev) || !aligned8(X_next_team_dev))
    return fail(DPGO_ERR_INVALID, "team: pointer not 8-byte aligned");
  if (!(grad_tol >= 0.0)) return fail(DPGO_ERR_INVALID, "certify: bad gradient tolerance");
  Team t;
  CHK(team_check(members_next, n_members, t));
  dpgo_problem_s* p0 = t.h[0];
  const int d = p0->d;
  if (!supported(d, r) || !supported(d, r + 1)) return fail(DPGO_ERR_UNSUPPORTED, "certify: (d, r + 1) not compiled in");
  if (p0->r != r + 1) return fail(DPGO_ERR_INVALID, "certify: the escape handles must have rank r + 1");
  *out = dpgo_team_escape_result{};
  CHK(team_tables(members_next, t, nullptr));
  TeamEval ev;
  CHK(ev.init());
  // f0 at alpha = 0: [X; 0] has the cost of X, and the tables hold nothing that depends on the rank
  double gn0 = 0.0;
  CHK(ev.run(t, d, r, X_team_dev, nullptr, &out->f_before, &gn0));
  const int g = std::min(pose_tiles(t.N, d + 1), kMaxGrid);
  double f = 0.0, gn = 0.0;  // of the last trial
  auto trial = [&](double a, double* f_out, double* gn_out) -> int {
    CHK(dispatch_dr(d, r + 1, [&](auto D, auto R1) {  // (by the rank it writes: only compiled lifts are instantiated)
      if constexpr (R1 > D)
        return launch(k_cert_lift_retract<D, R1 - 1>, g, 0, p0->stream, X_team_dev, witness_team_dev, a, X_next_team_dev, t.N);
      return fail(DPGO_ERR_UNSUPPORTED, "certify: no lift to rank d");
    }));
    HIPC(hipGetLastError());
    CHK(ev.run(t, d, r + 1, X_next_team_dev, nullptr, &f, &gn));
    *f_out = f;
    *gn_out = gn;
    return DPGO_OK;
  };
  CHK(halving_search(t.N, out->f_before, grad_tol, trial, &out->alpha, &out->trials));
  out->f_after = f;
  out->gradnorm_after = gn;
  return DPGO_OK;
}

}  // extern "C"
