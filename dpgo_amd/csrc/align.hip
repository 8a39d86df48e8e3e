// align.hip -- frame alignment of agents that start in their own frames (kernels/align.h): C ABI entries.
#include "host.h"

namespace {

int edge_grid(int m) { return std::max(1, std::min(kMaxGrid, (m + kBlock - 1) / kBlock)); }

// YLift (r x d column-major, host) as a kernel argument
LiftArg lift_arg(const double* YLift_host, int r, int d) {
  LiftArg y;
  std::memset(&y, 0, sizeof(y));
  std::memcpy(y.v, YLift_host, sizeof(double) * (size_t)r * d);
  return y;
}

// the caller's parameters with the defaults resolved, or an error
int average_args(int d, const dpgo_average_params* prm, AverageArgs* out) {
  if (d != 2 && d != 3) return fail(DPGO_ERR_INVALID, "d must be 2 or 3");
  if (!prm) return fail(DPGO_ERR_INVALID, "null parameters");
  if (prm->mode != DPGO_AVERAGE_TWO_STAGE && prm->mode != DPGO_AVERAGE_POSE) return fail(DPGO_ERR_INVALID, "unknown mode");
  if (!(prm->barc > 0.0) || !(prm->mu_step > 0.0) || !(prm->w_tol > 0.0) || !(prm->mu_cap > 0.0))
    return fail(DPGO_ERR_INVALID, "barc, mu_step, mu_cap and w_tol must be positive");
  if (prm->max_iterations < 0 || prm->min_inliers < 0) return fail(DPGO_ERR_INVALID, "negative max_iterations / min_inliers");
  const bool pose = prm->mode == DPGO_AVERAGE_POSE;
  out->mode = pose ? kAvgPose : kAvgTwoStage;
  out->barc = prm->barc;
  out->mu_step = prm->mu_step;
  out->mu_cap = prm->mu_cap;
  out->w_tol = prm->w_tol;
  out->max_iterations = prm->max_iterations > 0 ? prm->max_iterations : (pose ? 10000 : 1000);
  out->min_inliers = prm->min_inliers;
  out->kappa = pose ? 1.82 : 1.0;
  out->tau = pose ? 0.01 : 1.0;
  return DPGO_OK;
}

}  // namespace

static_assert(sizeof(AverageRecord) == sizeof(dpgo_average_result), "the device record is dpgo_average_result");

extern "C" {

void dpgo_average_params_default(int mode, dpgo_average_params* p) {
  if (!p) return;
  const bool pose = mode == DPGO_AVERAGE_POSE;
  p->mode = pose ? DPGO_AVERAGE_POSE : DPGO_AVERAGE_TWO_STAGE;
  // angular2ChordalSO3(0.5) = 2 sqrt(2) sin(0.25) (src/DPGO_utils.cpp:514-516); sqrt(chi2inv(0.9, 3))
  p->barc = pose ? std::sqrt(6.251388631170325) : 2.0 * std::sqrt(2.0) * std::sin(0.25);
  p->mu_step = 1.4;
  p->mu_cap = 1e-5;
  p->w_tol = 1e-8;
  p->max_iterations = 0;
  p->min_inliers = 2;
}


int dpgo_neighbor_candidates_device(int r, int d, int m, const double* YLift_host, const double* T_local_dev,
                                    const double* nbr_tiles_dev, const int32_t* my_pose_dev, const int32_t* slot_dev,
                                    const uint8_t* incoming_dev, const double* R_dev, const double* t_dev,
                                    double* cand_dev, void* stream) {
  if (d != 2 && d != 3) return fail(DPGO_ERR_INVALID, "d must be 2 or 3");
  if (!supported(d, r)) return fail(DPGO_ERR_UNSUPPORTED, "unsupported (d, r)");
  if (m < 0) return fail(DPGO_ERR_INVALID, "m < 0");
  if (m == 0) return DPGO_OK;
  if (!YLift_host || !T_local_dev || !nbr_tiles_dev || !my_pose_dev || !slot_dev || !incoming_dev || !R_dev || !t_dev ||
      !cand_dev)
    return fail(DPGO_ERR_INVALID, "null pointer");
  if (!aligned8(T_local_dev) || !aligned8(nbr_tiles_dev) || !aligned8(R_dev) || !aligned8(t_dev) || !aligned8(cand_dev) ||
      ((uintptr_t)my_pose_dev & 3) || ((uintptr_t)slot_dev & 3))
    return fail(DPGO_ERR_INVALID, "misaligned pointer");
  const LiftArg y = lift_arg(YLift_host, r, d);
  CHK(dispatch_dr(d, r, [&](auto D, auto R) {
    return launch(k_neighbor_candidates<D, R>, edge_grid(m), 0, (hipStream_t)stream, y, T_local_dev, nbr_tiles_dev,
                  my_pose_dev, slot_dev, incoming_dev, R_dev, t_dev, cand_dev, m);
  }));
  HIPC(hipGetLastError());
  return DPGO_OK;
}


int dpgo_robust_average_device(int d, int ngroups, const int32_t* group_ptr_dev, const double* cand_dev,
                               const double* kappa_dev, const double* tau_dev, const dpgo_average_params* params,
                               double* weights_dev, dpgo_average_result* results_dev, void* stream) {
  AverageArgs a;
  CHK(average_args(d, params, &a));
  if (ngroups < 0) return fail(DPGO_ERR_INVALID, "ngroups < 0");
  if (ngroups == 0) return DPGO_OK;
  if (!group_ptr_dev || !cand_dev || !weights_dev || !results_dev) return fail(DPGO_ERR_INVALID, "null pointer");
  if (((uintptr_t)group_ptr_dev & 3) || !aligned8(cand_dev) || !aligned8(kappa_dev) || !aligned8(tau_dev) ||
      !aligned8(weights_dev) || !aligned8(results_dev))
    return fail(DPGO_ERR_INVALID, "misaligned pointer");
  AverageRecord* rec = reinterpret_cast<AverageRecord*>(results_dev);
  if (d == 2)
    launch(k_robust_average<2>, ngroups, 0, (hipStream_t)stream, group_ptr_dev, cand_dev, kappa_dev, tau_dev, a, weights_dev, rec);
  else
    launch(k_robust_average<3>, ngroups, 0, (hipStream_t)stream, group_ptr_dev, cand_dev, kappa_dev, tau_dev, a, weights_dev, rec);
  HIPC(hipGetLastError());
  return DPGO_OK;
}


int dpgo_robust_average(int d, int ngroups, const int32_t* group_ptr, const double* cand, const double* kappa,
                        const double* tau, const dpgo_average_params* params, double* weights,
                        dpgo_average_result* results, int device) {
  AverageArgs a;
  CHK(average_args(d, params, &a));
  if (ngroups < 0) return fail(DPGO_ERR_INVALID, "ngroups < 0");
  if (ngroups == 0) return DPGO_OK;
  if (!group_ptr || !results) return fail(DPGO_ERR_INVALID, "null pointer");
  if (group_ptr[0] < 0) return fail(DPGO_ERR_INVALID, "group_ptr[0] < 0");
  for (int g = 0; g < ngroups; ++g)
    if (group_ptr[g + 1] < group_ptr[g]) return fail(DPGO_ERR_INVALID, "group_ptr decreases");
  const size_t m = (size_t)group_ptr[ngroups];
  if (m > 0 && (!cand || !weights)) return fail(DPGO_ERR_INVALID, "null pointer");
  int cnt = 0;
  CHK(dpgo_device_count(&cnt));
  if (cnt <= 0) return fail(DPGO_ERR_HIP, "no HIP device (this library has no CPU fallback)");
  if (device < 0 || device >= cnt) return fail(DPGO_ERR_INVALID, "device index out of range");
  HIPC(hipSetDevice(device));
  const size_t ts = (size_t)(d + 1) * d;
  DevBuf<int32_t> gp;
  DevBuf<double> c, k, t, w;
  DevBuf<dpgo_average_result> res;
  CHK(upload(gp, group_ptr, (size_t)ngroups + 1, nullptr));
  CHK(upload(c, cand, m * ts, nullptr));
  if (kappa) CHK(upload(k, kappa, m, nullptr));
  if (tau) CHK(upload(t, tau, m, nullptr));
  CHK(w.alloc(m > 0 ? m : 1));
  CHK(res.alloc(ngroups));
  CHK(dpgo_robust_average_device(d, ngroups, gp, c, kappa ? k.get() : nullptr, tau ? t.get() : nullptr, params, w, res,
                                 nullptr));
  if (m > 0) HIPC(hipMemcpy(weights, w, sizeof(double) * m, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(results, res, sizeof(dpgo_average_result) * (size_t)ngroups, hipMemcpyDeviceToHost));
  return DPGO_OK;
}


int dpgo_lift_in_frame_device(int r, int d, int n, const double* YLift_host, const double* T_local_dev,
                              const dpgo_average_result* result_dev, const double* T_world_robot_host, double* X_dev,
                              void* stream) {
  if (d != 2 && d != 3) return fail(DPGO_ERR_INVALID, "d must be 2 or 3");
  if (!supported(d, r)) return fail(DPGO_ERR_UNSUPPORTED, "unsupported (d, r)");
  if (n <= 0) return fail(DPGO_ERR_INVALID, "n <= 0");
  if (!YLift_host || !T_local_dev || !X_dev) return fail(DPGO_ERR_INVALID, "null pointer");
  if ((result_dev == nullptr) == (T_world_robot_host == nullptr))
    return fail(DPGO_ERR_INVALID, "exactly one of result_dev and T_world_robot_host must be given");
  if (!aligned8(T_local_dev) || !aligned8(X_dev) || !aligned8(result_dev)) return fail(DPGO_ERR_INVALID, "misaligned pointer");
  const LiftArg y = lift_arg(YLift_host, r, d);
  FrameArg f;
  std::memset(&f, 0, sizeof(f));
  f.use = T_world_robot_host ? 1 : 0;
  if (T_world_robot_host) std::memcpy(f.v, T_world_robot_host, sizeof(double) * (size_t)(d + 1) * d);
  const AverageRecord* rec = reinterpret_cast<const AverageRecord*>(result_dev);
  CHK(dispatch_dr(d, r, [&](auto D, auto R) {
    return launch(k_lift_in_frame<D, R>, edge_grid(n), 0, (hipStream_t)stream, y, T_local_dev, rec, f, X_dev, n);
  }));
  HIPC(hipGetLastError());
  return DPGO_OK;
}

}  // extern "C"
