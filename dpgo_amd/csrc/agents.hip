// agents.hip -- callers either side of the local solve: GNC and robust-cost re-weighting (src/DPGO_robust.cpp, src/PGOAgent.cpp:997-1142), initial guesses (src/DPGO_solver.cpp:220-303), manifold operations (src/manifold/*.cpp), public-pose exchange plans.
#include "host.h"

namespace dpgo_host {

int rebuild_vals(dpgo_problem_s* p, int nnzb, const int32_t* cptr, const int32_t* cedge, const uint8_t* ckind,
                 const double* base, double sign, double* out) {
  if (nnzb <= 0) return DPGO_OK;
  const int g = std::max(1, std::min(kMaxGrid, (nnzb + kBlock - 1) / kBlock));
  if (p->d == 2)
    launch(k_rebuild_Q<2>, g, 0, p->stream, p->gnc.dev(), cptr, cedge, ckind, base, sign, out, nnzb);
  else
    launch(k_rebuild_Q<3>, g, 0, p->stream, p->gnc.dev(), cptr, cedge, ckind, base, sign, out, nnzb);
  HIPC(hipGetLastError());
  return DPGO_OK;
}
int rebuild_Q_from_weights(dpgo_problem_s* p, const double* base, double sign, double* out) {
  return rebuild_vals(p, p->Q.nnzb, p->gnc.c_ptr, p->gnc.c_edge, p->gnc.c_kind, base, sign, out);
}
int rebuild_C_from_weights(dpgo_problem_s* p, const double* base, double sign, double* out) {
  if (!p->gnc.g_ptr) return DPGO_OK;
  return rebuild_vals(p, p->C.nnzb, p->gnc.g_ptr, p->gnc.g_edge, p->gnc.g_kind, base, sign, out);
}
int refresh_after_weights(dpgo_problem_s* p) {
  CHK(rebuild_Q_from_weights(p, p->gnc.q_base, 1.0, p->Q.vals));
  CHK(rebuild_C_from_weights(p, p->gnc.c_base, 1.0, p->C.vals));  // G itself is refreshed by the next update_G call
  p->ml_ready = false;
  p->auto_decided = false;
  p->sym.ready = p->tcg_sym = false;
  const double s = p->dinv_shift > 0 ? p->dinv_shift : 1e-1;
  p->dinv_shift = -1.0;  // clearQuadraticMatrix also drops the preconditioner (src/PoseGraph.cpp:352-355)
  return build_dinv(p, s);
}
}  // namespace dpgo_host

extern "C" {


int dpgo_problem_set_reweightable_edges_ex(dpgo_problem_t p, int m, const int32_t* p1, const int32_t* p2,
                                           const uint8_t* role, const int32_t* slot_in, const double* R,
                                           const double* t, const double* kappa, const double* tau,
                                           const double* weight, const uint8_t* fixed_weight) {
  CHK(check_ready(p));
  if (m < 0 || (m > 0 && (!p1 || !p2 || !R || !t || !kappa || !tau || !weight || !fixed_weight)))
    return fail(DPGO_ERR_INVALID, "null edge arrays");
  if (role && !slot_in) return fail(DPGO_ERR_INVALID, "roles given without neighbour slots");
  const int n = p->n, d = p->d, nnzb = p->Q.nnzb;
  // host copy of the patterns to locate the blocks each edge contributes to
  std::vector<int32_t> rowptr(n + 1), colidx(nnzb);
  HIPC(hipMemcpy(rowptr.data(), p->Q.rowptr, sizeof(int32_t) * (n + 1), hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(colidx.data(), p->Q.colidx, sizeof(int32_t) * nnzb, hipMemcpyDeviceToHost));
  int n_shared = 0;
  for (int e = 0; e < m; ++e)
    if (role && role[e]) ++n_shared;
  std::vector<int32_t> crow, ccol;
  const int cnnz = (n_shared > 0) ? p->C.nnzb : 0;
  if (n_shared > 0) {
    if (!p->C.rowptr) return fail(DPGO_ERR_STATE, "shared re-weightable edges need the G coupling first");
    crow.resize(n + 1);
    ccol.resize(cnnz > 0 ? cnnz : 1);
    HIPC(hipMemcpy(crow.data(), p->C.rowptr, sizeof(int32_t) * (n + 1), hipMemcpyDeviceToHost));
    if (cnnz > 0) HIPC(hipMemcpy(ccol.data(), p->C.colidx, sizeof(int32_t) * cnnz, hipMemcpyDeviceToHost));
  }
  auto find = [](const std::vector<int32_t>& rp, const std::vector<int32_t>& ci, int i, int j) -> int {
    const int32_t* b = ci.data() + rp[i];
    const int32_t* e = ci.data() + rp[i + 1];
    const int32_t* it = std::lower_bound(b, e, (int32_t)j);
    return (it != e && *it == j) ? (int)(it - ci.data()) : -1;
  };
  std::vector<std::vector<std::pair<int, uint8_t>>> lists(nnzb), glists(cnnz);
  std::vector<uint8_t> role_v(m > 0 ? m : 1, 0);
  std::vector<int32_t> slot_v(m > 0 ? m : 1, 0);
  for (int e = 0; e < m; ++e) {
    const int i = p1[e], j = p2[e];
    const int ro = role ? role[e] : 0;
    role_v[e] = (uint8_t)ro;
    if (ro == 0) {
      if (i < 0 || i >= n || j < 0 || j >= n || i == j) return fail(DPGO_ERR_INVALID, "edge endpoint out of range");
      const int sii = find(rowptr, colidx, i, i), sjj = find(rowptr, colidx, j, j), sij = find(rowptr, colidx, i, j),
                sji = find(rowptr, colidx, j, i);
      if (sii < 0 || sjj < 0 || sij < 0 || sji < 0)
        return fail(DPGO_ERR_STATE, "edge does not fit the block pattern of Q");
      lists[sii].push_back({e, 0});
      lists[sjj].push_back({e, 1});
      lists[sij].push_back({e, 2});
      lists[sji].push_back({e, 3});
    } else if (ro == 1 || ro == 2) {
      // outgoing: Q_ii += T Om T^T, C(i, slot) = -T Om; incoming: Q_jj += Om, C(j, slot) = -Om T^T
      // (PoseGraph::constructQ :462-486, constructG :533-562)
      const int mine = (ro == 1) ? i : j;
      const int sl = slot_in[e];
      if (mine < 0 || mine >= n || sl < 0 || sl >= p->C.ncols)
        return fail(DPGO_ERR_INVALID, "shared edge endpoint / neighbour slot out of range");
      slot_v[e] = sl;
      const int sd = find(rowptr, colidx, mine, mine), sc = find(crow, ccol, mine, sl);
      if (sd < 0 || sc < 0) return fail(DPGO_ERR_STATE, "shared edge does not fit the pattern of Q / the G coupling");
      lists[sd].push_back({e, (uint8_t)(ro == 1 ? 0 : 1)});
      glists[sc].push_back({e, (uint8_t)(ro == 1 ? 2 : 3)});
    } else {
      return fail(DPGO_ERR_INVALID, "edge role must be 0, 1 or 2");
    }
  }
  auto flatten = [](const std::vector<std::vector<std::pair<int, uint8_t>>>& L, std::vector<int32_t>& ptr,
                    std::vector<int32_t>& edge, std::vector<uint8_t>& kind) {
    ptr.assign(L.size() + 1, 0);
    for (size_t s = 0; s < L.size(); ++s) {
      for (auto& pr : L[s]) {
        edge.push_back(pr.first);
        kind.push_back(pr.second);
      }
      ptr[s + 1] = (int32_t)edge.size();
    }
  };
  std::vector<int32_t> cptr, cedge, gptr, gedge;
  std::vector<uint8_t> ckind, gkind;
  flatten(lists, cptr, cedge, ckind);
  p->gnc = dpgo_problem_s::GncEdges();
  p->gnc.em = m;
  p->gnc.n_shared_edges = n_shared;
  CHK(upload(p->gnc.e_p1, p1, (size_t)m, p->stream));
  CHK(upload(p->gnc.e_p2, p2, (size_t)m, p->stream));
  CHK(upload(p->gnc.e_role, role_v.data(), (size_t)m, p->stream));
  CHK(upload(p->gnc.e_slot, slot_v.data(), (size_t)m, p->stream));
  CHK(upload(p->gnc.e_R, R, (size_t)m * d * d, p->stream));
  CHK(upload(p->gnc.e_t, t, (size_t)m * d, p->stream));
  CHK(upload(p->gnc.e_kappa, kappa, (size_t)m, p->stream));
  CHK(upload(p->gnc.e_tau, tau, (size_t)m, p->stream));
  CHK(upload(p->gnc.e_w, weight, (size_t)m, p->stream));
  CHK(upload(p->gnc.e_fixed, fixed_weight, (size_t)m, p->stream));
  CHK(upload(p->gnc.c_ptr, cptr.data(), cptr.size(), p->stream));
  CHK(upload(p->gnc.c_edge, cedge.data(), cedge.size(), p->stream));
  CHK(upload(p->gnc.c_kind, ckind.data(), ckind.size(), p->stream));
  CHK(p->gnc.e_rsq.alloc(m > 0 ? m : 1));
  CHK(p->gnc.q_base.alloc((size_t)nnzb * p->b * p->b));
  // base = Q(current weights) - sum of the listed edges' contributions at those weights
  CHK(rebuild_Q_from_weights(p, p->Q.vals, -1.0, p->gnc.q_base));
  if (n_shared > 0 && cnnz > 0) {
    flatten(glists, gptr, gedge, gkind);
    CHK(upload(p->gnc.g_ptr, gptr.data(), gptr.size(), p->stream));
    CHK(upload(p->gnc.g_edge, gedge.data(), gedge.size(), p->stream));
    CHK(upload(p->gnc.g_kind, gkind.data(), gkind.size(), p->stream));
    CHK(p->gnc.c_base.alloc((size_t)cnnz * p->b * p->b));
    CHK(rebuild_C_from_weights(p, p->C.vals, -1.0, p->gnc.c_base));
  }
  HIPC(hipStreamSynchronize(p->stream));
  return DPGO_OK;
}


int dpgo_problem_set_reweightable_edges(dpgo_problem_t p, int m, const int32_t* p1, const int32_t* p2, const double* R,
                                        const double* t, const double* kappa, const double* tau, const double* weight,
                                        const uint8_t* fixed_weight) {
  return dpgo_problem_set_reweightable_edges_ex(p, m, p1, p2, nullptr, nullptr, R, t, kappa, tau, weight,
                                                fixed_weight);
}


// The result record of k_edge_robust_finish is read back as a dpgo_reweight_stats
static_assert(sizeof(RobustStatsDev) == sizeof(dpgo_reweight_stats) && offsetof(dpgo_reweight_stats, inliers) == 0 &&
                  offsetof(dpgo_reweight_stats, skipped) == 3 * sizeof(int) &&
                  offsetof(dpgo_reweight_stats, max_rsq) == offsetof(RobustStatsDev, max_rsq) &&
                  offsetof(dpgo_reweight_stats, cost) == offsetof(RobustStatsDev, cost),
              "RobustStatsDev mirrors dpgo_reweight_stats");
static_assert(DPGO_COST_L2 == kCostL2 && DPGO_COST_L1 == kCostL1 && DPGO_COST_TLS == kCostTLS &&
                  DPGO_COST_HUBER == kCostHuber && DPGO_COST_GM == kCostGM && DPGO_COST_GNC_TLS == kCostGncTls,
              "cost type numbers of the header and of the kernel");

// What both re-weighting entries do once their arguments are checked: k_edge_robust over the registered edges, its
// workgroups' records summed by k_edge_robust_finish, the values of Q / coupling / preconditioner rebuilt if the weights
// changed, and the one result record read back.
static int reweight_on_stream(dpgo_problem_t p, const double* X_dev, const double* nbr, const RobustCostDev& c,
                              double w_tol, int update, RobustStatsDev* out) {
  if (!p->gnc.r_partial) CHK(p->gnc.r_partial.alloc(kMaxGrid));
  if (!p->gnc.r_stats) CHK(p->gnc.r_stats.alloc(1));
  int g = std::max(1, std::min(kMaxGrid, (p->gnc.em + kBlock - 1) / kBlock));
  if (options().grid_edges > 0) g = std::min(g, options().grid_edges);
  CHK(dispatch_dr(p->d, p->r, [&](auto D, auto R) {
    return launch(k_edge_robust<D, R>, g, 0, p->stream, p->gnc.dev(), X_dev, nbr, c, w_tol, update, p->gnc.r_partial);
  }));
  launch(k_edge_robust_finish, 1, 0, p->stream, p->gnc.r_partial, g, p->gnc.r_stats);
  HIPC(hipGetLastError());
  if (update) CHK(refresh_after_weights(p));
  HIPC(hipMemcpyAsync(out, p->gnc.r_stats, sizeof(*out), hipMemcpyDeviceToHost, p->stream));
  HIPC(hipStreamSynchronize(p->stream));
  return DPGO_OK;
}


int dpgo_problem_gnc_reweight_device(dpgo_problem_t p, const double* X_dev, const double* nbr_tiles_dev, double mu,
                                     double barc, double w_tol, int update, int counts[3], double* max_rsq) {
  CHK(check_ready(p));
  if (!p->gnc.e_w) return fail(DPGO_ERR_STATE, "re-weightable edges not set");
  if (!X_dev) return fail(DPGO_ERR_INVALID, "null X");
  if (p->gnc.n_shared_edges > 0 && !nbr_tiles_dev) return fail(DPGO_ERR_INVALID, "shared edges need the neighbour tiles");
  if (update && !(mu > 0.0)) return fail(DPGO_ERR_INVALID, "GNC mu must be positive");
  // (without an update mu and barc reach the record's cost only, which this entry does not return)
  RobustStatsDev h{};
  CHK(reweight_on_stream(p, X_dev, nbr_tiles_dev, RobustCostDev{kCostGncTls, mu, barc, 0.0, 0.0}, w_tol, update, &h));
  if (counts) {
    counts[0] = h.n[0];
    counts[1] = h.n[1];
    counts[2] = h.n[2] + h.n[3];  // an edge whose weight was not stored (skipped) is not decided either
  }
  if (max_rsq) *max_rsq = h.max_rsq;
  return DPGO_OK;
}


int dpgo_problem_gnc_reweight(dpgo_problem_t p, const double* X_host, double mu, double barc, double w_tol, int update,
                              int counts[3], double* max_rsq) {
  CHK(check_ready(p));
  if (!X_host) return fail(DPGO_ERR_INVALID, "null X");
  if (p->gnc.n_shared_edges > 0) return fail(DPGO_ERR_STATE, "shared edges need the device flavour (neighbour tiles)");
  CHK(h2d(p, p->x2, X_host));
  return dpgo_problem_gnc_reweight_device(p, p->x2, nullptr, mu, barc, w_tol, update, counts, max_rsq);
}


void dpgo_robust_cost_default(dpgo_robust_cost* c) {
  if (!c) return;
  c->type = DPGO_COST_L2;
  c->mu = 1e-4;
  c->barc = 5.0;
  c->huber_threshold = 3.0;
  c->tls_threshold = 10.0;
}


int dpgo_problem_robust_reweight_device(dpgo_problem_t p, const double* X_dev, const double* nbr_tiles_dev,
                                        const dpgo_robust_cost* cost, double w_tol, int update, dpgo_reweight_stats* stats) {
  if (!p) {  // (no handle exists without a device: say so instead of "null handle")
    int cnt = 0;
    if (dpgo_device_count(&cnt) != DPGO_OK || cnt <= 0)
      return fail(DPGO_ERR_HIP, "no HIP device (this library has no CPU fallback)");
  }
  CHK(check_ready(p));
  if (!p->gnc.e_w) return fail(DPGO_ERR_STATE, "re-weightable edges not set");
  if (!X_dev || !cost || !stats) return fail(DPGO_ERR_INVALID, "null X / cost / stats");
  if (p->gnc.n_shared_edges > 0 && !nbr_tiles_dev) return fail(DPGO_ERR_INVALID, "shared edges need the neighbour tiles");
  if (std::isnan(w_tol)) return fail(DPGO_ERR_INVALID, "w_tol is NaN");
  switch (cost->type) {
    case DPGO_COST_L2:
    case DPGO_COST_L1:
    case DPGO_COST_GM: break;
    case DPGO_COST_HUBER:
      if (!(cost->huber_threshold > 0.0)) return fail(DPGO_ERR_INVALID, "Huber threshold must be positive");
      break;
    case DPGO_COST_TLS:
      if (!(cost->tls_threshold > 0.0)) return fail(DPGO_ERR_INVALID, "TLS threshold must be positive");
      break;
    case DPGO_COST_GNC_TLS:
      if (!(cost->mu > 0.0) || !(cost->barc > 0.0)) return fail(DPGO_ERR_INVALID, "GNC mu and barc must be positive");
      break;
    default: return fail(DPGO_ERR_INVALID, "unknown robust cost type");
  }
  RobustStatsDev h{};
  CHK(reweight_on_stream(p, X_dev, nbr_tiles_dev,
                         RobustCostDev{cost->type, cost->mu, cost->barc, cost->huber_threshold, cost->tls_threshold}, w_tol,
                         update, &h));
  std::memcpy(stats, &h, sizeof(h));
  return DPGO_OK;
}


int dpgo_problem_robust_reweight(dpgo_problem_t p, const double* X_host, const dpgo_robust_cost* cost, double w_tol,
                                 int update, dpgo_reweight_stats* stats) {
  if (!p) return dpgo_problem_robust_reweight_device(p, nullptr, nullptr, cost, w_tol, update, stats);
  CHK(check_ready(p));
  if (!X_host) return fail(DPGO_ERR_INVALID, "null X");
  if (p->gnc.n_shared_edges > 0) return fail(DPGO_ERR_STATE, "shared edges need the device flavour (neighbour tiles)");
  CHK(h2d(p, p->x2, X_host));
  return dpgo_problem_robust_reweight_device(p, p->x2, nullptr, cost, w_tol, update, stats);
}


int dpgo_problem_set_edge_weights(dpgo_problem_t p, const double* weight_host) {
  CHK(check_ready(p));
  if (!p->gnc.e_w) return fail(DPGO_ERR_STATE, "re-weightable edges not set");
  if (!weight_host) return fail(DPGO_ERR_INVALID, "null weights");
  if (p->gnc.em > 0) HIPC(hipMemcpyAsync(p->gnc.e_w, weight_host, sizeof(double) * p->gnc.em, hipMemcpyHostToDevice, p->stream));
  CHK(refresh_after_weights(p));
  HIPC(hipStreamSynchronize(p->stream));
  return DPGO_OK;
}


int dpgo_problem_get_edge_weights(dpgo_problem_t p, double* weight_host, double* rsq_host) {
  CHK(check_ready(p));
  if (!p->gnc.e_w) return fail(DPGO_ERR_STATE, "re-weightable edges not set");
  if (weight_host && p->gnc.em > 0)
    HIPC(hipMemcpyAsync(weight_host, p->gnc.e_w, sizeof(double) * p->gnc.em, hipMemcpyDeviceToHost, p->stream));
  if (rsq_host && p->gnc.em > 0)
    HIPC(hipMemcpyAsync(rsq_host, p->gnc.e_rsq, sizeof(double) * p->gnc.em, hipMemcpyDeviceToHost, p->stream));
  HIPC(hipStreamSynchronize(p->stream));
  return DPGO_OK;
}


// ---- initial guesses ----
namespace {
// Masked PCG: solve  mask A mask x = rhs  (rhs already masked) for the tiles x; A = the handle's Q.  Host-driven
// (two tiny read-backs per iteration): initialisation runs once per problem, outside the hot path.
struct InitBufs {
  DevBuf<double> x, r, z, p, Ap, diag, partial;
};
int init_dot(dpgo_problem_s* h, const double* a, const double* b, InitBufs& w, size_t total, int g, double* out) {
  launch(k_init_dot, g, 0, h->stream, a, b, w.partial, total);
  HIPC(hipGetLastError());
  std::vector<double> host(g);
  HIPC(hipMemcpyAsync(host.data(), w.partial, sizeof(double) * g, hipMemcpyDeviceToHost, h->stream));
  HIPC(hipStreamSynchronize(h->stream));
  double s = 0.0;
  for (double v : host) s += v;
  *out = s;
  return DPGO_OK;
}
int init_pcg(dpgo_problem_s* h, InitBufs& w, const double* rhs, int mode, double tol, int max_iter, int* iters) {
  const int T = h->T, R = h->r, D = h->d;
  const size_t total = (size_t)h->n * T;
  const int g = std::max(1, std::min(kMaxGrid, (int)((total + kBlock - 1) / kBlock)));
  auto axpby = [&](double a, const double* x, double b, double* y) -> int {
    launch(k_init_axpby, g, 0, h->stream, a, x, b, y, total, T, R, D, mode);
    HIPC(hipGetLastError());
    return DPGO_OK;
  };
  auto apply = [&](const double* v, double* out) -> int {  // out = mask(A v), v masked
    CHK(launch_spmm(h, h->Q, v, nullptr, out));
    return axpby(1.0, out, 0.0, out);
  };
  auto precond = [&](const double* r, double* z) -> int {
    launch(k_init_jacobi, g, 0, h->stream, r, w.diag, z, total, T, R, D, mode);
    HIPC(hipGetLastError());
    return DPGO_OK;
  };
  HIPC(hipMemsetAsync(w.x, 0, sizeof(double) * total, h->stream));
  CHK(axpby(1.0, rhs, 0.0, w.r));
  CHK(precond(w.r, w.z));
  CHK(axpby(1.0, w.z, 0.0, w.p));
  double rz = 0.0, r0 = 0.0;
  CHK(init_dot(h, w.r, w.z, w, total, g, &rz));
  CHK(init_dot(h, w.r, w.r, w, total, g, &r0));
  *iters = 0;
  if (!(r0 > 0.0)) return DPGO_OK;
  double best = r0;
  for (int it = 0; it < max_iter; ++it) {
    CHK(apply(w.p, w.Ap));
    double pAp = 0.0;
    CHK(init_dot(h, w.p, w.Ap, w, total, g, &pAp));
    if (!(pAp > 0.0)) break;
    const double alpha = rz / pAp;
    CHK(axpby(alpha, w.p, 1.0, w.x));
    CHK(axpby(-alpha, w.Ap, 1.0, w.r));
    CHK(precond(w.r, w.z));
    double rz_new = 0.0, rr = 0.0;
    CHK(init_dot(h, w.r, w.z, w, total, g, &rz_new));
    CHK(init_dot(h, w.r, w.r, w, total, g, &rr));
    *iters = it + 1;
    best = std::min(best, rr);
    if (rr <= tol * tol * r0) break;
    CHK(axpby(1.0, w.z, rz_new / rz, w.p));
    rz = rz_new;
  }
  return DPGO_OK;
}
}  // namespace


int dpgo_chordal_initialization(int d, int n, int m, const int32_t* p1, const int32_t* p2, const double* R,
                                const double* t, const double* kappa, const double* tau, double tol, int max_iter,
                                double* T_host, int iters_out[2], int device) {
  if ((d != 2 && d != 3) || n <= 0 || m < 0 || !T_host || (m > 0 && (!p1 || !p2 || !R || !t || !kappa || !tau)))
    return fail(DPGO_ERR_INVALID, "bad arguments");
  if (!(tol > 0.0)) tol = 1e-13;
  if (max_iter <= 0) max_iter = (int)std::min<long long>(20ll * n + 100, 200000);
  const int b = d + 1, r = d;  // tiles [n][d+1][d]: the rank-d "lifted" problem IS the SE(d) problem
  std::vector<int32_t> zero(std::max(m, 1), 0);
  std::vector<double> ones(std::max(m, 1), 1.0), tau0(std::max(m, 1), 0.0);
  dpgo_problem_t hq[2] = {nullptr, nullptr};  // [0]: rotation-only connection Laplacian (tau = 0), [1]: Q
  struct Cleanup {
    dpgo_problem_t* h;
    ~Cleanup() {
      dpgo_problem_destroy(h[0]);
      dpgo_problem_destroy(h[1]);
    }
  } cleanup{hq};
  for (int which = 0; which < 2; ++which) {
    const double* tw = which == 0 ? tau0.data() : tau;
    int nnzb = 0;
    int rc = dpgo_build_Q_bsr(0, d, n, m, zero.data(), p1, zero.data(), p2, R, t, kappa, tw, ones.data(), 0, nullptr, 0.0,
                              0.0, &nnzb, nullptr, nullptr, nullptr);
    if (rc != DPGO_OK) return fail(rc, "chordal initialisation: measurement index out of range");
    std::vector<int32_t> rowptr(n + 1), colidx(nnzb);
    std::vector<double> vals((size_t)nnzb * b * b);
    rc = dpgo_build_Q_bsr(0, d, n, m, zero.data(), p1, zero.data(), p2, R, t, kappa, tw, ones.data(), 0, nullptr, 0.0, 0.0,
                          &nnzb, rowptr.data(), colidx.data(), vals.data());
    if (rc != DPGO_OK) return fail(rc, "chordal initialisation: could not build the data matrix");
    CHK(dpgo_problem_create(&hq[which], r, d, n, device));
    CHK(dpgo_problem_set_Q_bsr(hq[which], nnzb, rowptr.data(), colidx.data(), vals.data()));
  }
  dpgo_problem_s* hr = hq[0];
  dpgo_problem_s* ht = hq[1];
  const size_t total = (size_t)n * hr->T;
  InitBufs w;
  DevBuf<double> rhs, V, Tr;
  for (DevBuf<double>* v : {&w.x, &w.r, &w.z, &w.p, &w.Ap, &rhs, &V, &Tr}) CHK(v->alloc(total));
  CHK(w.diag.alloc((size_t)n * b));
  CHK(w.partial.alloc(kMaxGrid));
  const int gflat = std::max(1, std::min(kMaxGrid, (n + kBlock - 1) / kBlock));
  const int gtot = std::max(1, std::min(kMaxGrid, (int)((total + kBlock - 1) / kBlock)));
  int it_rot = 0, it_tr = 0;
  // ---- rotations: minimise sum kappa |R_j - R_i R_ij|^2, R_0 = I.  With E0 = tile 0 = [I | 0]:  L (E0 + x) = 0 on
  // the free rows  =>  mask L mask x = -mask(L E0)
  std::vector<double> e0(hr->T, 0.0);
  for (int c = 0; c < d; ++c) e0[(size_t)c * r + c] = 1.0;
  HIPC(hipMemsetAsync(V, 0, sizeof(double) * total, hr->stream));
  HIPC(hipStreamSynchronize(hr->stream));  // (the host copy below comes from pageable memory: keep it strictly after)
  HIPC(hipMemcpyAsync(V, e0.data(), sizeof(double) * hr->T, hipMemcpyHostToDevice, hr->stream));
  HIPC(hipStreamSynchronize(hr->stream));
  CHK(launch_spmm(hr, hr->Q, V, nullptr, rhs));
  launch(k_init_axpby, gtot, 0, hr->stream, -1.0, rhs, 0.0, rhs, total, hr->T, r, d, 0);
  if (d == 2)
    launch(k_init_diag<2>, gflat, 0, hr->stream, hr->Q.dev(), w.diag, n);
  else
    launch(k_init_diag<3>, gflat, 0, hr->stream, hr->Q.dev(), w.diag, n);
  HIPC(hipGetLastError());
  CHK(init_pcg(hr, w, rhs, 0, tol, max_iter, &it_rot));
  // V = E0 + x, then every block to SO(d) (projectToRotationGroup, src/DPGO_utils.cpp:464-478): the rounding kernel with
  // the identity as anchor
  launch(k_init_axpby, gtot, 0, hr->stream, 1.0, w.x, 0.0, w.x, total, hr->T, r, d, 0);
  HIPC(hipMemcpyAsync(V, w.x, sizeof(double) * total, hipMemcpyDeviceToDevice, hr->stream));
  HIPC(hipStreamSynchronize(hr->stream));  // (as above)
  HIPC(hipMemcpyAsync(V, e0.data(), sizeof(double) * hr->T, hipMemcpyHostToDevice, hr->stream));
  HIPC(hipStreamSynchronize(hr->stream));
  CHK(dpgo_round_trajectory_device(r, d, n, V, e0.data(), Tr, hr->stream));
  HIPC(hipStreamSynchronize(hr->stream));
  // ---- translations: minimise sum tau |t_j - t_i - R_i t_ij|^2, t_0 = 0: the translation columns of Q [R | t] = 0
  CHK(launch_spmm(ht, ht->Q, Tr, nullptr, rhs));
  launch(k_init_axpby, gtot, 0, ht->stream, -1.0, rhs, 0.0, rhs, total, ht->T, r, d, 1);
  if (d == 2)
    launch(k_init_diag<2>, gflat, 0, ht->stream, ht->Q.dev(), w.diag, n);
  else
    launch(k_init_diag<3>, gflat, 0, ht->stream, ht->Q.dev(), w.diag, n);
  HIPC(hipGetLastError());
  CHK(init_pcg(ht, w, rhs, 1, tol, max_iter, &it_tr));
  // T = [R | t]: rotation columns from Tr, translation column from the solve (pose 0: zero)
  launch(k_init_axpby, gtot, 0, ht->stream, 1.0, w.x, 0.0, w.x, total, ht->T, r, d, 1);
  launch(k_axpby_plain, gtot, 0, ht->stream, 1.0, w.x, 1.0, Tr, total);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(T_host, Tr, sizeof(double) * total, hipMemcpyDeviceToHost, ht->stream));
  HIPC(hipStreamSynchronize(ht->stream));
  if (iters_out) {
    iters_out[0] = it_rot;
    iters_out[1] = it_tr;
  }
  return DPGO_OK;
}


int dpgo_odometry_initialization(int d, int n, int m, const int32_t* p1, const int32_t* p2, const double* R,
                                 const double* t, double* T_host) {
  if ((d != 2 && d != 3) || n <= 0 || m < 0 || !T_host || (m > 0 && (!p1 || !p2 || !R || !t)))
    return fail(DPGO_ERR_INVALID, "bad arguments");
  const int b = d + 1;
  std::vector<int> edge_of(n, -1);  // odometry edge leaving pose i (i -> i + 1)
  for (int e = 0; e < m; ++e)
    if (p1[e] >= 0 && p1[e] + 1 == p2[e] && p2[e] < n && edge_of[p1[e]] < 0) edge_of[p1[e]] = e;
  std::memset(T_host, 0, sizeof(double) * (size_t)n * b * d);
  for (int c = 0; c < d; ++c) T_host[(size_t)c * d + c] = 1.0;  // tile 0 = [I | 0]
  for (int dst = 1; dst < n; ++dst) {
    const int e = edge_of[dst - 1];
    if (e < 0) return fail(DPGO_ERR_INVALID, "odometry initialisation: no odometry edge " + std::to_string(dst - 1) +
                                                 " -> " + std::to_string(dst));  // reference: CHECK(m.p1 == src)
    const double* Ts = T_host + (size_t)(dst - 1) * b * d;  // tile [c][row]: R(row, c) at c*d + row, t(row) at d*d + row
    double* Td = T_host + (size_t)dst * b * d;
    const double* Re = R + (size_t)e * d * d;  // R[e][row][col]
    const double* te = t + (size_t)e * d;
    for (int row = 0; row < d; ++row) {
      for (int c = 0; c < d; ++c) {
        double s = 0.0;
        for (int k = 0; k < d; ++k) s += Ts[(size_t)k * d + row] * Re[k * d + c];  // (R_src R_e)(row, c)
        Td[(size_t)c * d + row] = s;
      }
      double s = Ts[(size_t)d * d + row];
      for (int k = 0; k < d; ++k) s += Ts[(size_t)k * d + row] * te[k];  // t_src + R_src t_e
      Td[(size_t)d * d + row] = s;
    }
  }
  return DPGO_OK;
}


// ---- manifold ----
namespace {
int manifold_args(int r, int d, int n, int device) {
  if (n <= 0 || r < d || d < 2 || d > 3) return fail(DPGO_ERR_INVALID, "need n > 0, r >= d, d in {2,3}");
  if (!supported(d, r)) return fail(DPGO_ERR_UNSUPPORTED, "(d, r) not compiled in");
  int cnt = 0;
  CHK(dpgo_device_count(&cnt));
  if (cnt <= 0) return fail(DPGO_ERR_HIP, "no HIP device (this library has no CPU fallback)");
  if (device < 0 || device >= cnt) return fail(DPGO_ERR_INVALID, "device index out of range");
  HIPC(hipSetDevice(device));
  return DPGO_OK;
}
int tiles_grid(int d, int n) { return std::min(kMaxGrid, pose_tiles(n, d + 1)); }
}  // namespace


int dpgo_manifold_project_device(int r, int d, int n, const double* M_dev, double* out_dev, void* stream) {
  return dpgo_axpby_project_device(r, d, n, 1.0, M_dev, 0.0, nullptr, 0.0, nullptr, 1, out_dev, stream);
}


int dpgo_axpby_project_device(int r, int d, int n, double a, const double* A_dev, double b, const double* B_dev,
                              double c, const double* C_dev, int project, double* out_dev, void* stream) {
  if (!A_dev || !out_dev) return fail(DPGO_ERR_INVALID, "null pointer");
  if (n <= 0) return fail(DPGO_ERR_INVALID, "n <= 0");
  CHK(dispatch_dr(d, r, [&](auto D, auto R) {
    return launch(k_axpby_project<D, R>, tiles_grid(d, n), 0, (hipStream_t)stream, a, A_dev, b, B_dev, c, C_dev, project,
                  out_dev, n);
  }));
  HIPC(hipGetLastError());
  return DPGO_OK;
}


int dpgo_round_trajectory_device(int r, int d, int n, const double* X_dev, const double* anchor_host, double* T_dev,
                                 void* stream) {
  if (!X_dev || !T_dev) return fail(DPGO_ERR_INVALID, "null pointer");
  if (n <= 0) return fail(DPGO_ERR_INVALID, "n <= 0");
  if (!dpgo_supported(d, r)) return fail(DPGO_ERR_UNSUPPORTED, "unsupported (d, r)");
  AnchorArg an;
  std::memset(&an, 0, sizeof(an));
  an.use = anchor_host ? 1 : 0;
  if (anchor_host) std::memcpy(an.v, anchor_host, sizeof(double) * (size_t)(d + 1) * r);
  int g = (n + kBlock - 1) / kBlock;
  if (g > kMaxGrid) g = kMaxGrid;
  CHK(dispatch_dr(d, r, [&](auto D, auto R) {
    return launch(k_round<D, R>, g, 0, (hipStream_t)stream, X_dev, an, T_dev, n);
  }));
  HIPC(hipGetLastError());
  return DPGO_OK;
}


int dpgo_round_trajectory(int r, int d, int n, const double* X_host, const double* anchor_host, double* T_host,
                          int device) {
  if (!X_host || !T_host) return fail(DPGO_ERR_INVALID, "null pointer");
  CHK(manifold_args(r, d, n, device));
  const size_t xb = sizeof(double) * (size_t)n * (d + 1) * r, tb = sizeof(double) * (size_t)n * (d + 1) * d;
  DevBuf<double> X, T;
  CHK(X.alloc((size_t)n * (d + 1) * r));
  CHK(T.alloc((size_t)n * (d + 1) * d));
  HIPC(hipMemcpy(X, X_host, xb, hipMemcpyHostToDevice));
  CHK(dpgo_round_trajectory_device(r, d, n, X, anchor_host, T, nullptr));
  HIPC(hipMemcpy(T_host, T, tb, hipMemcpyDeviceToHost));
  return DPGO_OK;
}


int dpgo_gather_tiles_device(int r, int d, const double* src_dev, const int32_t* idx_dev, int count, double* dst_dev,
                             void* stream) {
  if (count == 0) return DPGO_OK;
  if (!src_dev || !idx_dev || !dst_dev || count < 0) return fail(DPGO_ERR_INVALID, "bad arguments");
  size_t total = (size_t)count * (d + 1) * r;
  int g = (int)((total + kBlock - 1) / kBlock);
  if (g > kMaxGrid) g = kMaxGrid;
  CHK(dispatch_dr(d, r, [&](auto D, auto R) {
    return launch(k_gather_tiles<D, R>, g, 0, (hipStream_t)stream, src_dev, idx_dev, count, dst_dev);
  }));
  HIPC(hipGetLastError());
  return DPGO_OK;
}


int dpgo_permute_tiles_device(int r, int d, int n, const int32_t* new_index_dev, const double* in_dev, double* out_dev,
                              int forward, void* stream) {
  if (n == 0) return DPGO_OK;
  if (!new_index_dev || !in_dev || !out_dev || n < 0 || in_dev == out_dev) return fail(DPGO_ERR_INVALID, "bad arguments");
  size_t total = (size_t)n * (d + 1) * r;
  int g = (int)((total + kBlock - 1) / kBlock);
  if (g > kMaxGrid) g = kMaxGrid;
  CHK(dispatch_dr(d, r, [&](auto D, auto R) {
    return launch(forward ? k_scatter_tiles<D, R> : k_gather_tiles<D, R>, g, 0, (hipStream_t)stream, in_dev, new_index_dev, n,
                  out_dev);
  }));
  HIPC(hipGetLastError());
  return DPGO_OK;
}


struct dpgo_exchange_plan_s {
  int device = 0, T = 0, nmsg = 0, total = 0;
  DevBuf<const double*> src;
  DevBuf<const int32_t*> idx;
  DevBuf<double*> dst;
  DevBuf<int32_t> first;
};


int dpgo_exchange_plan_create(dpgo_exchange_plan_t* out, int r, int d, int nmsg, const double* const* src_dev,
                              const int32_t* const* idx_dev, const int* count, double* const* dst_dev, int device) {
  if (!out || nmsg <= 0 || !src_dev || !idx_dev || !count || !dst_dev || !supported(d, r))
    return fail(DPGO_ERR_INVALID, "bad exchange plan arguments");
  *out = nullptr;
  std::vector<int32_t> first(nmsg + 1, 0);
  for (int m = 0; m < nmsg; ++m) {
    if (count[m] < 0 || (count[m] > 0 && (!src_dev[m] || !idx_dev[m] || !dst_dev[m]))) return fail(DPGO_ERR_INVALID, "bad message");
    first[m + 1] = first[m] + count[m];
  }
  HIPC(hipSetDevice(device));
  auto* pl = new dpgo_exchange_plan_s();
  pl->device = device;
  pl->T = (d + 1) * r;
  pl->nmsg = nmsg;
  pl->total = first[nmsg];
  int rc = [&]() -> int {
    CHK(pl->src.alloc(nmsg));
    CHK(pl->idx.alloc(nmsg));
    CHK(pl->dst.alloc(nmsg));
    CHK(pl->first.alloc(nmsg + 1));
    HIPC(hipMemcpy(pl->src, src_dev, sizeof(void*) * nmsg, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(pl->idx, idx_dev, sizeof(void*) * nmsg, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(pl->dst, dst_dev, sizeof(void*) * nmsg, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(pl->first, first.data(), sizeof(int32_t) * (nmsg + 1), hipMemcpyHostToDevice));
    return DPGO_OK;
  }();
  if (rc != DPGO_OK) {
    dpgo_exchange_plan_destroy(pl);
    return rc;
  }
  *out = pl;
  return DPGO_OK;
}


int dpgo_exchange_plan_run(dpgo_exchange_plan_t pl, void* stream) {
  if (!pl) return fail(DPGO_ERR_INVALID, "null exchange plan");
  if (pl->total == 0) return DPGO_OK;
  HIPC(hipSetDevice(pl->device));
  const ExchangeTable tb{pl->src, pl->idx, pl->dst, pl->first, pl->nmsg};
  const int g = std::max(1, std::min(kMaxGrid, (pl->total + kBlock / 4 - 1) / (kBlock / 4)));
  switch (pl->T) {
#define CASE_T(TT) case TT: launch(k_gather_tiles_batched<TT>, g, 0, (hipStream_t)stream, tb); break;
    CASE_T(6) CASE_T(9) CASE_T(12) CASE_T(15) CASE_T(16) CASE_T(20) CASE_T(24)
#undef CASE_T
    default: return fail(DPGO_ERR_UNSUPPORTED, "unsupported (d, r)");
  }
  HIPC(hipGetLastError());
  return DPGO_OK;
}


// ---- ordering words of the peer-store transport (kernels/agent.h: k_flags_write / k_flags_wait) ----
// (a table longer than kFlagCap goes out in several launches: a null word anywhere is refused before the first of them)
static int flag_words_ok(int n, unsigned long long* const* words_dev) {
  for (int k = 0; k < n; ++k)
    if (!words_dev[k]) return fail(DPGO_ERR_INVALID, "null ordering word");
  return DPGO_OK;
}
static int flag_table(int n, unsigned long long* const* words_dev, const unsigned long long* values, int first, FlagTable* t) {
  t->n = std::min(kFlagCap, n - first);
  for (int k = 0; k < t->n; ++k) {
    t->p[k] = words_dev[first + k];
    t->v[k] = values[first + k];
  }
  return DPGO_OK;
}
int dpgo_flags_write_device(int n, unsigned long long* const* words_dev, const unsigned long long* values, void* stream) {
  if (n < 0 || (n > 0 && (!words_dev || !values))) return fail(DPGO_ERR_INVALID, "bad ordering-word arguments");
  CHK(flag_words_ok(n, words_dev));
  for (int first = 0; first < n; first += kFlagCap) {
    FlagTable t;
    CHK(flag_table(n, words_dev, values, first, &t));
    launch_wg(k_flags_write, 1, dim3(64), 0, (hipStream_t)stream, t);
  }
  HIPC(hipGetLastError());
  return DPGO_OK;
}
namespace {
int flags_wait(int n, unsigned long long* const* words_dev, const unsigned long long* values, long long timeout_ms,
               unsigned long long* err_word, void* stream) {
  CHK(flag_words_ok(n, words_dev));
  for (int first = 0; first < n; first += kFlagCap) {
    FlagTable t;
    CHK(flag_table(n, words_dev, values, first, &t));
    launch_wg(k_flags_wait, 1, dim3(64), 0, (hipStream_t)stream, t, timeout_ms * 100000LL, err_word);
  }
  HIPC(hipGetLastError());
  return DPGO_OK;
}
}  // namespace
int dpgo_flags_wait_device(int n, unsigned long long* const* words_dev, const unsigned long long* values, int timeout_ms,
                           void* stream) {
  if (n < 0 || (n > 0 && (!words_dev || !values)) || timeout_ms <= 0) return fail(DPGO_ERR_INVALID, "bad ordering-word arguments");
  return flags_wait(n, words_dev, values, timeout_ms, nullptr, stream);
}
int dpgo_flags_wait_device_checked(int n, unsigned long long* const* words_dev, const unsigned long long* values,
                                   long long timeout_ms, unsigned long long* err_word, void* stream) {
  if (n < 0 || (n > 0 && (!words_dev || !values)) || timeout_ms < 0 || (timeout_ms > 0 && !err_word))
    return fail(DPGO_ERR_INVALID, "bad ordering-word arguments");
  return flags_wait(n, words_dev, values, timeout_ms, err_word, stream);
}

int dpgo_exchange_plan_destroy(dpgo_exchange_plan_t pl) {
  delete pl;
  return DPGO_OK;
}


int dpgo_max_translation_distance_device(int r, int d, int n, const double* X_dev, const double* Xprev_dev,
                                         double* out_dev, double* out_host, void* stream) {
  if (!X_dev || !Xprev_dev || !out_dev || n <= 0) return fail(DPGO_ERR_INVALID, "bad arguments");
  hipStream_t s = (hipStream_t)stream;
  HIPC(hipMemsetAsync(out_dev, 0, sizeof(double), s));
  const int g = std::max(1, std::min(kMaxGrid, (n + kBlock - 1) / kBlock));
  CHK(dispatch_dr(d, r, [&](auto D, auto R) {
    return launch(k_max_translation_distance<D, R>, g, 0, s, X_dev, Xprev_dev, n,
                  reinterpret_cast<unsigned long long*>(out_dev));
  }));
  HIPC(hipGetLastError());
  if (out_host) {
    HIPC(hipMemcpyAsync(out_host, out_dev, sizeof(double), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
  }
  return DPGO_OK;
}


int dpgo_manifold_project(int r, int d, int n, const double* M, double* out, int device) {
  if (!M || !out) return fail(DPGO_ERR_INVALID, "null pointer");
  CHK(manifold_args(r, d, n, device));
  const size_t total = (size_t)n * (d + 1) * r, vb = sizeof(double) * total;
  DevBuf<double> a, o;
  CHK(a.alloc(total));
  CHK(o.alloc(total));
  HIPC(hipMemcpy(a, M, vb, hipMemcpyHostToDevice));
  CHK(dpgo_manifold_project_device(r, d, n, a, o, nullptr));
  HIPC(hipMemcpy(out, o, vb, hipMemcpyDeviceToHost));
  return DPGO_OK;
}


int dpgo_manifold_tangent_project(int r, int d, int n, const double* X, const double* V, double* out, int device) {
  if (!X || !V || !out) return fail(DPGO_ERR_INVALID, "null pointer");
  CHK(manifold_args(r, d, n, device));
  const size_t total = (size_t)n * (d + 1) * r, vb = sizeof(double) * total;
  DevBuf<double> x, v, o;
  for (DevBuf<double>* q : {&x, &v, &o}) CHK(q->alloc(total));
  HIPC(hipMemcpy(x, X, vb, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(v, V, vb, hipMemcpyHostToDevice));
  CHK(dispatch_dr(d, r, [&](auto D, auto R) {
    return launch(k_precond<D, R>, tiles_grid(d, n), 0, nullptr, x, v, nullptr, o, n);
  }));
  HIPC(hipGetLastError());
  HIPC(hipMemcpy(out, o, vb, hipMemcpyDeviceToHost));
  return DPGO_OK;
}


int dpgo_manifold_retract(int r, int d, int n, const double* X, const double* eta, double scale, double* out,
                          int device) {
  if (!X || !eta || !out) return fail(DPGO_ERR_INVALID, "null pointer");
  CHK(manifold_args(r, d, n, device));
  const size_t total = (size_t)n * (d + 1) * r, vb = sizeof(double) * total;
  DevBuf<double> x, v, o;
  for (DevBuf<double>* q : {&x, &v, &o}) CHK(q->alloc(total));
  HIPC(hipMemcpy(x, X, vb, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(v, eta, vb, hipMemcpyHostToDevice));
  CHK(dispatch_dr(d, r, [&](auto D, auto R) {
    return launch(k_retract<D, R>, tiles_grid(d, n), 0, nullptr, x, v, scale, o, nullptr, n, nullptr, nullptr, nullptr, nullptr,
                  nullptr, nullptr);
  }));
  HIPC(hipGetLastError());
  HIPC(hipMemcpy(out, o, vb, hipMemcpyDeviceToHost));
  return DPGO_OK;
}

}  // extern "C"
