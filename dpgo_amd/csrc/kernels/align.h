// kernels/align.h -- frame alignment of an agent that starts in its own frame: candidate transforms from the shared loop closures, their robust (GNC-TLS) average, the lift of the local trajectory into the global frame.
// Part of kernels.h (included inside namespace dpgo, behind agent.h: it uses robust_weight, jacobi_columns and block_allreduce).
#pragma once

// Small rigid transforms in registers: Rm[row][col], t[row].  Pose::inverse and Pose::operator* of the reference
// (include/DPGO/manifold/Poses.h:200-209): inv(R, t) = (R^T, -R^T t), (Ra, ta) (Rb, tb) = (Ra Rb, Ra tb + ta).
template <int D>
struct Rigid {
  double Rm[D][D];
  double t[D];
};
template <int D>
__device__ __forceinline__ Rigid<D> rigid_inverse(const Rigid<D>& a) {
  Rigid<D> o;
#pragma unroll
  for (int p = 0; p < D; ++p) {
#pragma unroll
    for (int q = 0; q < D; ++q) o.Rm[p][q] = a.Rm[q][p];
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) s = fma(a.Rm[k][p], a.t[k], s);
    o.t[p] = -s;
  }
  return o;
}
template <int D>
__device__ __forceinline__ Rigid<D> rigid_compose(const Rigid<D>& a, const Rigid<D>& b) {
  Rigid<D> o;
#pragma unroll
  for (int p = 0; p < D; ++p) {
#pragma unroll
    for (int q = 0; q < D; ++q) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) s = fma(a.Rm[p][k], b.Rm[k][q], s);
      o.Rm[p][q] = s;
    }
    double s = a.t[p];
#pragma unroll
    for (int k = 0; k < D; ++k) s = fma(a.Rm[p][k], b.t[k], s);
    o.t[p] = s;
  }
  return o;
}
// tile [D+1][D] (the D columns of the rotation, then the translation: what k_round writes) <-> Rigid
template <int D>
__device__ __forceinline__ Rigid<D> rigid_load(const double* __restrict__ tile) {
  Rigid<D> o;
#pragma unroll
  for (int c = 0; c < D; ++c)
#pragma unroll
    for (int a = 0; a < D; ++a) o.Rm[a][c] = tile[c * D + a];
#pragma unroll
  for (int a = 0; a < D; ++a) o.t[a] = tile[D * D + a];
  return o;
}
template <int D>
__device__ __forceinline__ void rigid_store(double* __restrict__ tile, const Rigid<D>& v) {
#pragma unroll
  for (int c = 0; c < D; ++c)
#pragma unroll
    for (int a = 0; a < D; ++a) tile[c * D + a] = v.Rm[a][c];
#pragma unroll
  for (int a = 0; a < D; ++a) tile[D * D + a] = v.t[a];
}

// YLift (r x d, column-major: v[a * R + k] = YLift(k, a), the first d columns of a pose tile), by value as AnchorArg is
struct LiftArg {
  double v[3 * 6];
};
// a rigid transform given by the host (tile [d+1][d]); use == 0: the transform comes from a record in device memory
struct FrameArg {
  double v[4 * 3];
  int use;
};

// ================================================================ candidate frame transforms
// PGOAgent::computeNeighborTransform (src/PGOAgent.cpp:515-548), one lane per shared loop closure e, no projection and no
// check:   T_world2_world1 = (YLift^T X_nbr) * inv(T_frame1_frame2) * inv(T_world1_frame1)        (:530, :544-545)
// with T_frame1_frame2 = dT for an outgoing edge (my pose is p1) and inv(dT) for an incoming one (:535-543), X_nbr the
// neighbour's public pose nbr[slot[e]] (tile [D+1][R]) and T_world1_frame1 my pose T_local[my_pose[e]] in my own frame.
template <int D, int R>
__global__ __launch_bounds__(kBlock) void k_neighbor_candidates(LiftArg Y, const double* __restrict__ T_local,
                                                                const double* __restrict__ nbr,
                                                                const int32_t* __restrict__ my_pose,
                                                                const int32_t* __restrict__ slot,
                                                                const uint8_t* __restrict__ incoming,
                                                                const double* __restrict__ Rm, const double* __restrict__ tv,
                                                                double* __restrict__ cand, int m) {
  constexpr int B = D + 1;
  for (int e = blockIdx.x * kBlock + threadIdx.x; e < m; e += gridDim.x * kBlock) {
    const double* __restrict__ x = nbr + (size_t)slot[e] * (B * R);
    Rigid<D> w2f2;  // YLift^T X_nbr
#pragma unroll
    for (int a = 0; a < D; ++a) {
#pragma unroll
      for (int c = 0; c < D; ++c) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < R; ++k) s = fma(Y.v[a * R + k], x[c * R + k], s);
        w2f2.Rm[a][c] = s;
      }
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < R; ++k) s = fma(Y.v[a * R + k], x[D * R + k], s);
      w2f2.t[a] = s;
    }
    Rigid<D> dT;
#pragma unroll
    for (int a = 0; a < D; ++a) {
#pragma unroll
      for (int c = 0; c < D; ++c) dT.Rm[a][c] = Rm[(size_t)e * D * D + a * D + c];
      dT.t[a] = tv[(size_t)e * D + a];
    }
    Rigid<D> f1f2 = dT;
    if (incoming[e]) f1f2 = rigid_inverse<D>(dT);
    const Rigid<D> w1f1 = rigid_load<D>(T_local + (size_t)my_pose[e] * (B * D));
    const Rigid<D> w2f1 = rigid_compose<D>(w2f2, rigid_inverse<D>(f1f2));
    const Rigid<D> w2w1 = rigid_compose<D>(w2f1, rigid_inverse<D>(w1f1));
    rigid_store<D>(cand + (size_t)e * (B * D), w2w1);
  }
}

// ================================================================ robust average of the candidates of one group
// robustSingleRotationAveraging (src/DPGO_solver.cpp:72-135) and robustSinglePoseAveraging (:137-218), restated step by
// step; one workgroup per group of candidates [group_ptr[g], group_ptr[g+1]) and the whole GNC loop inside the kernel:
//   estimate with all weights 1 -> residuals -> muInit = barc^2 / (2 max rSq - barc^2), min(muInit, mu_cap) (:95-98);
//   muInit <= 0: no GNC, all weights stay 1, 0 iterations (:99-100);
//   else, at most max_iterations times: estimate with the current weights (:109), weights = RobustCost::weight(sqrt(rSq))
//   of GNC_TLS (src/DPGO_robust.cpp:80-92), stop when every weight is < w_tol or > 1 - w_tol (:115-122), else mu *= mu_step.
// The estimate returned is the one of the LAST solve (not recomputed with the final weights); inliers are w > 1 - w_tol.
// An estimate is singleRotationAveraging (:42-57: projectToRotationGroup of sum w kappa R) and, in pose mode,
// singleTranslationAveraging (:23-40: sum w tau t / sum w tau).  Two-stage mode (PGOAgent::
// computeRobustNeighborTransformTwoStage, src/PGOAgent.cpp:579-594) runs GNC on the rotations alone and then takes the
// plain mean of the inliers' translations.
// Sums: lane t adds candidates t, t + kBlock, .. in index order, block_allreduce adds the lanes in its fixed tree, so every
// lane holds the same bits, every branch below is uniform across the workgroup and two launches give the same bits.
// Unlike the reference: a group with a non-finite candidate entry (or precision) gets status INVALID before iterating
// (checkRotationMatrix would abort; a NaN would otherwise spin to the iteration cap), an empty group gets EMPTY, and a
// group with fewer inliers than min_inliers (two-stage mode: or none at all, which leaves no translation) gets FEW_INLIERS
// -- its transform is still reported.  Every loop is bounded by max_iterations; no workgroup waits for another.
constexpr int kAvgOk = 0, kAvgEmpty = 1, kAvgInvalid = 2, kAvgFewInliers = 3;
constexpr int kAvgTwoStage = 0, kAvgPose = 1;
struct AverageArgs {
  int mode;
  double barc, mu_step, mu_cap, w_tol;
  int max_iterations, min_inliers;
  double kappa, tau;  // used when the per-candidate arrays are NULL
};
// field for field dpgo_average_result (include/dpgo_hip.h)
struct AverageRecord {
  int status, inliers, candidates, iterations;
  double mu;
  double T[4 * 3];  // tile [d+1][d]
};

// projectToRotationGroup (src/DPGO_utils.cpp:464-478) of the D x D block whose COLUMNS are col[b][0..D): the rule of k_round
// (one-sided Jacobi M V = U diag(sigma); det V = +1, so the smallest column is negated when det U < 0).  rot[c][a] = R(a, c).
template <int D>
__device__ __forceinline__ void rotation_of_columns(double (&col)[D][D], double (&rot)[D][D]) {
  double V[D][D], nrm2[D], inv[D];
  jacobi_columns<D, D>(col, V);
  jacobi_inv_norms<D, D>(col, nrm2, inv);
  int kmin = 0;
#pragma unroll
  for (int k = 1; k < D; ++k) kmin = (nrm2[k] < nrm2[kmin]) ? k : kmin;
#pragma unroll
  for (int k = 0; k < D; ++k)
#pragma unroll
    for (int a = 0; a < D; ++a) col[k][a] *= inv[k];
  double det;
  if constexpr (D == 2) {
    det = col[0][0] * col[1][1] - col[0][1] * col[1][0];
  } else {
    det = col[0][0] * (col[1][1] * col[2][2] - col[1][2] * col[2][1]) -
          col[0][1] * (col[1][0] * col[2][2] - col[1][2] * col[2][0]) +
          col[0][2] * (col[1][0] * col[2][1] - col[1][1] * col[2][0]);
  }
  if (det < 0.0) {
#pragma unroll
    for (int k = 0; k < D; ++k)
#pragma unroll
      for (int a = 0; a < D; ++a) col[k][a] = (k == kmin) ? -col[k][a] : col[k][a];
  }
#pragma unroll
  for (int c = 0; c < D; ++c)
#pragma unroll
    for (int a = 0; a < D; ++a) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) s = fma(col[k][a], V[c][k], s);
      rot[c][a] = s;
    }
}

// One estimate: est = tile [D+1][D] of (projectToRotationGroup(sum w kappa R), sum w tau t / sum w tau).  first: all weights 1.
template <int D>
__device__ __forceinline__ void average_solve(const double* __restrict__ cand, const double* __restrict__ kappa,
                                              const double* __restrict__ tau, const double* weights, int lo, int n,
                                              bool first, const AverageArgs& A, double* red, double (&est)[(D + 1) * D]) {
  constexpr int TS = (D + 1) * D, K = TS + 1;
  double acc[K];
#pragma unroll
  for (int q = 0; q < K; ++q) acc[q] = 0.0;
  for (int i = lo + (int)threadIdx.x; i < lo + n; i += kBlock) {
    const double* __restrict__ c = cand + (size_t)i * TS;
    const double w = first ? 1.0 : weights[i];
    const double kw = (kappa ? kappa[i] : A.kappa) * w, tw = (tau ? tau[i] : A.tau) * w;
#pragma unroll
    for (int q = 0; q < D * D; ++q) acc[q] = fma(kw, c[q], acc[q]);
#pragma unroll
    for (int q = D * D; q < TS; ++q) acc[q] = fma(tw, c[q], acc[q]);
    acc[TS] += tw;
  }
  block_allreduce<K>(acc, red);
  double col[D][D], rot[D][D];
#pragma unroll
  for (int b = 0; b < D; ++b)
#pragma unroll
    for (int a = 0; a < D; ++a) col[b][a] = acc[b * D + a];
  rotation_of_columns<D>(col, rot);
#pragma unroll
  for (int b = 0; b < D; ++b)
#pragma unroll
    for (int a = 0; a < D; ++a) est[b * D + a] = rot[b][a];
#pragma unroll
  for (int a = 0; a < D; ++a) est[D * D + a] = acc[D * D + a] / acc[TS];
}

// rSq of one candidate against the estimate: kappa |R - R_i|_F^2 (+ tau |t - t_i|^2 in pose mode)
template <int D>
__device__ __forceinline__ double average_residual(const double* __restrict__ c, const double (&est)[(D + 1) * D],
                                                   double kap, double ta, bool pose) {
  double rot = 0.0, tr = 0.0;
#pragma unroll
  for (int q = 0; q < D * D; ++q) {
    const double v = est[q] - c[q];
    rot = fma(v, v, rot);
  }
#pragma unroll
  for (int q = D * D; q < (D + 1) * D; ++q) {
    const double v = est[q] - c[q];
    tr = fma(v, v, tr);
  }
  return pose ? kap * rot + ta * tr : kap * rot;
}

// (sum of cnt, maximum of mx) over the workgroup, the same bits in every lane; redmax: kWaves doubles
__device__ __forceinline__ void block_count_and_max(double& cnt, double& mx, double* red, double* redmax) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
  __syncthreads();  // (whoever still reads redmax of the call before is done)
  if ((threadIdx.x & 63) == 0) redmax[threadIdx.x >> 6] = mx;
  double c1[1] = {cnt};
  block_allreduce<1>(c1, red);  // (its barriers also order redmax)
  cnt = c1[0];
  double m = redmax[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) m = fmax(m, redmax[w]);
  mx = m;
}

template <int D>
__global__ __launch_bounds__(kBlock) void k_robust_average(const int32_t* __restrict__ group_ptr,
                                                           const double* __restrict__ cand,
                                                           const double* __restrict__ kappa,
                                                           const double* __restrict__ tau, AverageArgs A,
                                                           double* weights, AverageRecord* __restrict__ results) {
  constexpr int TS = (D + 1) * D;
  __shared__ double red[kWaves * (TS + 1)];
  __shared__ double redmax[kWaves];
  const int g = blockIdx.x;
  const int lo = group_ptr[g], n = group_ptr[g + 1] - lo;
  const bool pose = A.mode == kAvgPose;
  AverageRecord* __restrict__ out = results + g;
  double est[TS];
#pragma unroll
  for (int q = 0; q < TS; ++q) est[q] = 0.0;
  int status = kAvgOk, iterations = 0, inliers = 0;
  double mu = 0.0;
  if (n <= 0) {
    status = kAvgEmpty;
  } else {
    // weights start at 1 (:81); candidates and precisions must be finite
    double bad = 0.0, unused = 0.0;
    for (int i = lo + (int)threadIdx.x; i < lo + n; i += kBlock) {
      weights[i] = 1.0;
      const double* __restrict__ c = cand + (size_t)i * TS;
      bool ok = __builtin_isfinite(kappa ? kappa[i] : A.kappa) && __builtin_isfinite(tau ? tau[i] : A.tau);
#pragma unroll
      for (int q = 0; q < TS; ++q) ok = ok && __builtin_isfinite(c[q]);
      if (!ok) bad += 1.0;
    }
    block_count_and_max(bad, unused, red, redmax);
    if (bad > 0.0) {
      status = kAvgInvalid;
      for (int i = lo + (int)threadIdx.x; i < lo + n; i += kBlock) weights[i] = 0.0;
    } else {
      // initial estimate and its largest residual (:88-93)
      average_solve<D>(cand, kappa, tau, weights, lo, n, true, A, red, est);
      double cnt = 0.0, mx = 0.0;
      for (int i = lo + (int)threadIdx.x; i < lo + n; i += kBlock)
        mx = fmax(mx, average_residual<D>(cand + (size_t)i * TS, est, kappa ? kappa[i] : A.kappa, tau ? tau[i] : A.tau, pose));
      block_count_and_max(cnt, mx, red, redmax);
      const double bSq = A.barc * A.barc;
      mu = fmin(bSq / (2.0 * mx - bSq), A.mu_cap);
      if (mu > 0.0) {
        RobustCostDev cost;
        cost.type = kCostGncTls;
        cost.barc = A.barc;
        cost.huber = cost.tls = 0.0;
        for (int iter = 0; iter < A.max_iterations; ++iter) {
          average_solve<D>(cand, kappa, tau, weights, lo, n, false, A, red, est);
          cost.mu = mu;
          double nc = 0.0;
          mx = 0.0;
          for (int i = lo + (int)threadIdx.x; i < lo + n; i += kBlock) {
            const double rSq =
                average_residual<D>(cand + (size_t)i * TS, est, kappa ? kappa[i] : A.kappa, tau ? tau[i] : A.tau, pose);
            const double w = robust_weight(cost, rSq);
            if (w < A.w_tol || w > 1.0 - A.w_tol) nc += 1.0;
            mx = fmax(mx, rSq);
            weights[i] = w;  // (read back by this lane only: average_solve walks the same candidates)
          }
          block_count_and_max(nc, mx, red, redmax);
          iterations = iter + 1;
          if ((int)nc == n) break;
          mu *= A.mu_step;
        }
      }
      // inliers (:127-134); two-stage: the mean of their translations (src/PGOAgent.cpp:589-594)
      double tin[D + 1];
#pragma unroll
      for (int q = 0; q <= D; ++q) tin[q] = 0.0;
      for (int i = lo + (int)threadIdx.x; i < lo + n; i += kBlock) {
        if (weights[i] > 1.0 - A.w_tol) {
          const double* __restrict__ c = cand + (size_t)i * TS;
#pragma unroll
          for (int q = 0; q < D; ++q) tin[q] += c[D * D + q];
          tin[D] += 1.0;
        }
      }
      block_allreduce<D + 1>(tin, red);
      inliers = (int)tin[D];
      if (!pose) {
#pragma unroll
        for (int q = 0; q < D; ++q) est[D * D + q] = inliers > 0 ? tin[q] / tin[D] : 0.0;
      }
      if (inliers < A.min_inliers || (!pose && inliers == 0)) status = kAvgFewInliers;
    }
  }
  if (threadIdx.x == 0) {
    out->status = status;
    out->inliers = inliers;
    out->candidates = n > 0 ? n : 0;
    out->iterations = iterations;
    out->mu = mu;
#pragma unroll
    for (int q = 0; q < 4 * 3; ++q) out->T[q] = q < TS ? est[q] : 0.0;
  }
}

// ================================================================ lift of the local trajectory into the global frame
// PGOAgent::initializeInGlobalFrame (src/PGOAgent.cpp:329-337): X_i = YLift * (T_world_robot * T_local_i), one lane per pose,
// whole columns stored.  T_world_robot is the transform of a record of k_robust_average in device memory -- a record whose
// status is not OK leaves X untouched -- or, host.use != 0, a transform the host gives (robot 0: the identity, :299-301).
template <int D, int R>
__global__ __launch_bounds__(kBlock) void k_lift_in_frame(LiftArg Y, const double* __restrict__ T_local,
                                                          const AverageRecord* __restrict__ rec, FrameArg host,
                                                          double* __restrict__ X, int n) {
  constexpr int B = D + 1;
  if (!host.use && rec->status != kAvgOk) return;
  double tw[B * D];
#pragma unroll
  for (int q = 0; q < B * D; ++q) tw[q] = host.use ? host.v[q] : rec->T[q];
  const Rigid<D> Tw = rigid_load<D>(tw);
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const Rigid<D> Ti = rigid_compose<D>(Tw, rigid_load<D>(T_local + (size_t)i * (B * D)));
    double* __restrict__ x = X + (size_t)i * (B * R);
#pragma unroll
    for (int c = 0; c < B; ++c) {
      double col[R];
#pragma unroll
      for (int k = 0; k < R; ++k) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < D; ++a) s = fma(Y.v[a * R + k], c < D ? Ti.Rm[a][c] : Ti.t[a], s);
        col[k] = s;
      }
      store_col<R>(x + c * R, col);
    }
  }
}
