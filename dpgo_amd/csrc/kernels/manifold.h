// kernels/manifold.h -- manifold operations: stand-alone preconditioner / projection, qf retraction, polar projection, rounding to SE(d).
// Part of kernels.h (included inside namespace dpgo, in this order: common.h, problem.h, tcg.h, persist.h, multilevel.h, dense.h, manifold.h, rtr.h, agent.h, init.h).
#pragma once

// ================================================================ K6: preconditioner (stand-alone)
// Z = proj_X( V * Dinv )   (QuadraticProblem::PreConditioner, src/QuadraticProblem.cpp:56-69, with
// the block-Jacobi factor in place of the CHOLMOD solve); dinv == nullptr -> Z = proj_X(V).
template <int D, int R>
__global__ __launch_bounds__(kBlock) void k_precond(const double* __restrict__ X, const double* __restrict__ V,
                                                    const double* __restrict__ dinv, double* __restrict__ Z,
                                                    int n) {
  using GEO = Geo<D, R>;
  __shared__ double sm[kWaves][3][GEO::G][GEO::T];
  const LaneId L = lane_id<D>();
  const int ntiles = (n + GEO::P - 1) / GEO::P;
  const TileIter ti_ = tile_iter(ntiles);
  for (int tile = ti_.first; tile < ti_.last; tile += ti_.step) {
    const int i = tile * GEO::P + L.wave * GEO::G + L.g;
    const bool ok = (L.g < GEO::G) && (i < n);
    const size_t off = (size_t)i * GEO::T + L.c * R;
    double* ys = ok ? &sm[L.wave][0][L.g][0] : nullptr;
    double* vs = ok ? &sm[L.wave][1][L.g][0] : nullptr;
    double* zs = ok ? &sm[L.wave][2][L.g][0] : nullptr;
    double v[R], x[R], z[R];
    if (ok) {
      load_col<R>(X + off, x);
      load_col<R>(V + off, v);
      store_col<R>(ys + L.c * R, x);
      store_col<R>(vs + L.c * R, v);
    }
    wave_sync();
    if (ok) {
      if (dinv) {
        jacobi_col<D, R>(vs, dinv + (size_t)i * GEO::BB + L.c * GEO::B, z);
      } else {
#pragma unroll
        for (int a = 0; a < R; ++a) z[a] = v[a];
      }
      store_col<R>(zs + L.c * R, z);
    }
    wave_sync();
    if (ok) {
      double out[R], s[D];
      proj_col<D, R>(ys, zs, L.c, z, out, s);
      store_col<R>(Z + off, out);
    }
    wave_sync();
  }
}

// ================================================================ K4: retraction
// X2 = R_X(scale * eta): Stiefel factor = Q of the thin QR of Y + eta with diag(R) > 0 (modified
// Gram-Schmidt; ROPTLIB Stiefel::qfRetraction), Euclidean factor p + eta.  Each lane c < D rebuilds
// q_0..q_c from the LDS tile (identical arithmetic in all lanes of the pose).
// RHO (the RTR step, scale = 1): eta is tCG's iterate, `r` its residual and `g` the gradient it started from.  tCG keeps
// r = g + H eta (k_tcg_update: r = g, then r += alpha H delta beside eta += alpha delta, boundary step included), so the two
// sums of the rho test come from the eta column this kernel loads anyway, without a pass over Q:
// partials: [0] <eta, r - g> = <eta, H eta>   [1] <eta, g>   (what k_hess writes for V = eta, Gdot = g; k_rtr_update)
// DEF (the RTR step of a solve that kept tCG's directions, kernels/tcg.h): eta is not loaded but formed here, in registers,
// from the K = coef[0] directions of the ring `dirs` (slot k = n * T doubles) and their step lengths coef[1 + k], in the
// order of the iterations and starting from +0 -- the bits of the running sum it replaces -- with the loads of
// kDirsInFlight slots requested before the first of them is used.  The sum is element-wise, so with an even tile size it
// runs in span layout (lane-linear 16-byte pieces of the wave's G poses, as the span kernels of tCG; the slots are read
// once: non-temporal loads) and reaches the lanes' (pose, column) layout through the LDS tile; odd tile sizes sum column
// by column.  `eta` is not read.  `eta_out` (null: nobody asks): eta for whoever reads tCG's iterate after the step -- the
// DPGO_RHO_EXACT tail, which applies H to it.
constexpr int kDirsInFlight = 4;
template <int D, int R, bool RHO = false, bool DEF = false>
__global__ __launch_bounds__(kBlock) void k_retract(const double* __restrict__ X, const double* __restrict__ eta,
                                                    double scale, double* __restrict__ X2,
                                                    const DevState* __restrict__ st, int n,
                                                    const double* __restrict__ r, const double* __restrict__ g,
                                                    double* __restrict__ partials, const double* __restrict__ dirs,
                                                    const double* __restrict__ coef, double* __restrict__ eta_out) {
  using GEO = Geo<D, R>;
  using SPN = Span<D, R, 1>;
  constexpr bool kSpanSum = DEF && SPN::kOk;
  __shared__ __attribute__((aligned(16))) double sm[kWaves][GEO::G][GEO::T];
  __shared__ double red[kWaves * kNP];  // (RHO only)
  if (st && st->rtr_stop) return;
  const LaneId L = lane_id<D>();
  const int ntiles = (n + GEO::P - 1) / GEO::P;
  [[maybe_unused]] double part[2] = {0.0, 0.0};
  [[maybe_unused]] int ndirs = 0;
  if constexpr (DEF) ndirs = (int)coef[0];
  [[maybe_unused]] const size_t slot = (size_t)n * GEO::T;
  const TileIter ti_ = tile_iter(ntiles);
  for (int tile = ti_.first; tile < ti_.last; tile += ti_.step) {
    const int i = tile * GEO::P + L.wave * GEO::G + L.g;
    const bool ok = (L.g < GEO::G) && (i < n);
    const size_t off = (size_t)i * GEO::T + L.c * R;
    double* as = ok ? &sm[L.wave][L.g][0] : nullptr;
    if constexpr (kSpanSum) {  // wave-cooperative: the wave's span of eta into its LDS tile
      const int lane = threadIdx.x & 63;
      const int p0 = tile * GEO::P + L.wave * GEO::G;
      const int npose = (n - p0) < GEO::G ? (n - p0) : GEO::G;
      const int valid = npose > 0 ? npose * GEO::T : 0;
      const size_t base = (size_t)p0 * GEO::T;
      dbl2 e2[SPN::NIT];
#pragma unroll
      for (int it = 0; it < SPN::NIT; ++it) e2[it].x = e2[it].y = 0.0;
      for (int k0 = 0; k0 < ndirs; k0 += kDirsInFlight) {
        dbl2 dv[kDirsInFlight][SPN::NIT];
#pragma unroll
        for (int q = 0; q < kDirsInFlight; ++q)
          if (k0 + q < ndirs) {
            const dbl2* d2 = reinterpret_cast<const dbl2*>(dirs + (size_t)(k0 + q) * slot + base);
#pragma unroll
            for (int it = 0; it < SPN::NIT; ++it)
              if (2 * (lane + 64 * it) < valid) dv[q][it] = ld_stream<1>(d2 + lane + 64 * it);
          }
#pragma unroll
        for (int q = 0; q < kDirsInFlight; ++q)
          if (k0 + q < ndirs) {
            const double c = coef[1 + k0 + q];
#pragma unroll
            for (int it = 0; it < SPN::NIT; ++it)
              if (2 * (lane + 64 * it) < valid) {
                e2[it].x = fma(c, dv[q][it].x, e2[it].x);
                e2[it].y = fma(c, dv[q][it].y, e2[it].y);
              }
          }
      }
#pragma unroll
      for (int it = 0; it < SPN::NIT; ++it) {
        const int pc = lane + 64 * it;
        if (2 * pc < valid) {
          reinterpret_cast<dbl2*>(&sm[L.wave][0][0])[pc] = e2[it];
          if (eta_out) st_stream<1>(reinterpret_cast<dbl2*>(eta_out + base) + pc, e2[it]);
        }
      }
      wave_sync();
    }
    double a[R];
    if (ok) {
      double x[R], e[R];
      load_col<R>(X + off, x);
      if constexpr (kSpanSum) {
        load_col<R>(as + L.c * R, e);  // (this lane's column of the tile: overwritten below by the same lane)
      } else if constexpr (DEF) {
#pragma unroll
        for (int k = 0; k < R; ++k) e[k] = 0.0;
        for (int k0 = 0; k0 < ndirs; k0 += kDirsInFlight) {
          double dl[kDirsInFlight][R];
#pragma unroll
          for (int q = 0; q < kDirsInFlight; ++q)
            if (k0 + q < ndirs) load_col<R>(dirs + (size_t)(k0 + q) * slot + off, dl[q]);
#pragma unroll
          for (int q = 0; q < kDirsInFlight; ++q)
            if (k0 + q < ndirs) {
              const double c = coef[1 + k0 + q];
#pragma unroll
              for (int k = 0; k < R; ++k) e[k] = fma(c, dl[q][k], e[k]);
            }
        }
        if (eta_out) store_col<R>(eta_out + off, e);
      } else {
        load_col<R>(eta + off, e);
      }
      if constexpr (RHO) {
        double rc[R], gc[R];
        load_col<R>(r + off, rc);
        load_col<R>(g + off, gc);
#pragma unroll
        for (int k = 0; k < R; ++k) {
          part[0] = fma(e[k], rc[k] - gc[k], part[0]);
          part[1] = fma(e[k], gc[k], part[1]);
        }
      }
#pragma unroll
      for (int k = 0; k < R; ++k) a[k] = fma(scale, e[k], x[k]);
      store_col<R>(as + L.c * R, a);
    }
    wave_sync();
    if (ok) {
      qf_col<D, R>(as, L.c, a);
      store_col<R>(X2 + off, a);
    }
    wave_sync();
  }
  if constexpr (RHO) store_partials<2>(part, partials, red);
}

// ================================================================ one-sided Jacobi (shared by K5 and K12)
// Hestenes' one-sided Jacobi on the D columns a[p][0..N) of an N x D block M, held in registers: the columns of a pair
// (p, q) are rotated by the angle taken from their own dot products (Golub & Van Loan, Matrix Computations, 4th ed.,
// Alg. 8.6.3 applied to columns) until every pair is orthogonal to kJacobiTol relative to the pair's norms.  On return
// a = M V = U diag(sigma): the column norms are the singular values, the normalised columns are U, and V (the product
// of the plane rotations, so det V = +1) is accumulated from the identity.  Nothing here forms M^T M, so the factors
// lose eps kappa(M) where the Gram route M (M^T M)^-1/2 lost eps kappa(M)^2.
// The block is first scaled by a power of two (exact) so that its largest entry lies in [1, 2): the dot products can
// then neither overflow nor underflow, and a column whose squared norm falls below kJacobiZero (sigma below 1e-90
// sigma_max) is numerically zero: it is left alone here and contributes nothing to U V^T (jacobi_inv_norms).
constexpr double kJacobiTol = 0x1p-50;    // 4 eps: below the round-off of an N-term dot product nothing is gained
constexpr double kJacobiZero = 0x1p-600;  // on the squared norm of a column of the scaled block
constexpr int kJacobiSweeps = 30;         // (convergence is quadratic; the bound guarantees termination)
template <int D, int N>
__device__ __forceinline__ void jacobi_columns(double (&a)[D][N], double (&V)[D][D]) {
  double mx = 0.0;
#pragma unroll
  for (int p = 0; p < D; ++p)
#pragma unroll
    for (int k = 0; k < N; ++k) mx = fmax(mx, fabs(a[p][k]));
  const int ex = (mx > 0.0 && mx < INFINITY) ? -ilogb(mx) : 0;
#pragma unroll
  for (int p = 0; p < D; ++p) {
#pragma unroll
    for (int k = 0; k < N; ++k) a[p][k] = ldexp(a[p][k], ex);
#pragma unroll
    for (int q = 0; q < D; ++q) V[p][q] = (p == q) ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < D; ++p)
#pragma unroll
      for (int q = p + 1; q < D; ++q) {
        double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          al = fma(a[p][k], a[p][k], al);
          be = fma(a[q][k], a[q][k], be);
          ga = fma(a[p][k], a[q][k], ga);
        }
        if (al > kJacobiZero && be > kJacobiZero && fabs(ga) > kJacobiTol * (sqrt(al) * sqrt(be))) {
          rotated = true;
          const double zeta = (be - al) / (2.0 * ga);
          const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
          const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
#pragma unroll
          for (int k = 0; k < N; ++k) {
            const double x = a[p][k], y = a[q][k];
            a[p][k] = cs * x - sn * y;
            a[q][k] = sn * x + cs * y;
          }
#pragma unroll
          for (int k = 0; k < D; ++k) {
            const double x = V[k][p], y = V[k][q];
            V[k][p] = cs * x - sn * y;
            V[k][q] = sn * x + cs * y;
          }
        }
      }
    if (!rotated) break;
  }
}
// nrm2[k] = |a_k|^2 and inv[k] = 1 / |a_k| of the columns jacobi_columns left; inv = 0 for a numerically zero column
template <int D, int N>
__device__ __forceinline__ void jacobi_inv_norms(const double (&a)[D][N], double (&nrm2)[D], double (&inv)[D]) {
#pragma unroll
  for (int p = 0; p < D; ++p) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) s = fma(a[p][k], a[p][k], s);
    nrm2[p] = s;
    inv[p] = s > kJacobiZero ? 1.0 / sqrt(s) : 0.0;
  }
}

// ================================================================ K5: polar projection
// LiftedSEManifold::project (src/manifold/LiftedSEManifold.cpp:34-45; JacobiSVD U V^T,
// src/DPGO_utils.cpp:480-486).  out = polar( a*A + b*Bm + c*Cm ) per pose when project != 0:
// U V^T = sum_k (a_k / |a_k|) v_k^T from the one-sided Jacobi of the r x d block itself (jacobi_columns); a column
// of norm 0 contributes 0, so a rank-deficient block maps to a finite partial isometry.  One lane per pose column;
// every lane c < D of a pose repeats the small factorisation on the LDS copy of the tile and writes its own column.
template <int D, int R>
__global__ __launch_bounds__(kBlock) void k_axpby_project(double a, const double* __restrict__ A, double b,
                                                          const double* __restrict__ Bm, double c,
                                                          const double* __restrict__ Cm, int project,
                                                          double* __restrict__ out, int n) {
  using GEO = Geo<D, R>;
  __shared__ double sm[kWaves][GEO::G][GEO::T];
  const LaneId L = lane_id<D>();
  const int ntiles = (n + GEO::P - 1) / GEO::P;
  const TileIter ti_ = tile_iter(ntiles);
  for (int tile = ti_.first; tile < ti_.last; tile += ti_.step) {
    const int i = tile * GEO::P + L.wave * GEO::G + L.g;
    const bool ok = (L.g < GEO::G) && (i < n);
    const size_t off = (size_t)i * GEO::T + L.c * R;
    double* ms = ok ? &sm[L.wave][L.g][0] : nullptr;
    double m[R];
    if (ok) {
#pragma unroll
      for (int k = 0; k < R; ++k) {
        double v = a * A[off + k];
        if (Bm) v = fma(b, Bm[off + k], v);
        if (Cm) v = fma(c, Cm[off + k], v);
        m[k] = v;
      }
      store_col<R>(ms + L.c * R, m);
    }
    wave_sync();
    if (ok) {
      if (project && L.c < D) {
        double col[D][R], V[D][D], nrm2[D], inv[D];
#pragma unroll
        for (int p = 0; p < D; ++p)
#pragma unroll
          for (int k = 0; k < R; ++k) col[p][k] = ms[p * R + k];
        jacobi_columns<D, R>(col, V);
        jacobi_inv_norms<D, R>(col, nrm2, inv);
        // out column c = sum_k u_k V[c][k]
#pragma unroll
        for (int k = 0; k < R; ++k) m[k] = 0.0;
#pragma unroll
        for (int p = 0; p < D; ++p) {
          double vcp = 0.0;
#pragma unroll
          for (int cc = 0; cc < D; ++cc) vcp = (cc == L.c) ? V[cc][p] : vcp;
          const double f = vcp * inv[p];
#pragma unroll
          for (int k = 0; k < R; ++k) m[k] = fma(col[p][k], f, m[k]);
        }
      }
      store_col<R>(out + off, m);
    }
    wave_sync();
  }
}

// ================================================================ K12: rounding to SE(d)
// PGOAgent::getTrajectoryInLocalFrame / getTrajectoryInGlobalFrame (src/PGOAgent.cpp:718-767):
//   T_i = [ projectToRotationGroup(Ya^T Y_i) | Ya^T p_i - t0 ],  t0 = Ya^T pa,
// anchor (Ya, pa) = the global anchor, or pose 0 of X (local frame).  projectToRotationGroup
// (src/DPGO_utils.cpp:464-478: U V^T, last column of U negated when det U det V < 0) is evaluated as
// sum_k s_k u_k v_k^T from the one-sided Jacobi of M = Ya^T Y_i itself (jacobi_columns: M V = U diag(sigma)).  The
// sign comes from the orthogonal factors, which are well conditioned however small sigma_min is: det V = +1 by
// construction (a product of plane rotations), so s_k = -1 on the SMALLEST column norm when det U < 0.  A column of
// norm 0 contributes 0.  One lane per pose; output tiles [n][d+1][d] (= the reference's d x (d+1)n column-major
// Matrix).
struct AnchorArg {
  double v[4 * 6];  // (d+1) x r tile, same layout as a pose tile of X
  int use;          // 0: take pose 0 of X
};
template <int D, int R>
__global__ __launch_bounds__(kBlock) void k_round(const double* __restrict__ X, AnchorArg anchor,
                                                  double* __restrict__ T, int n) {
  constexpr int B = D + 1, TS = B * R;
  double Ya[D][R], pa[R];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int k = 0; k < R; ++k) Ya[a][k] = anchor.use ? anchor.v[a * R + k] : X[a * R + k];
#pragma unroll
  for (int k = 0; k < R; ++k) pa[k] = anchor.use ? anchor.v[D * R + k] : X[D * R + k];
  double t0[D];
#pragma unroll
  for (int a = 0; a < D; ++a) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < R; ++k) s = fma(Ya[a][k], pa[k], s);
    t0[a] = s;
  }
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const double* __restrict__ x = X + (size_t)i * TS;
    double M[D][D], tt[D];
#pragma unroll
    for (int a = 0; a < D; ++a) {
#pragma unroll
      for (int b = 0; b < D; ++b) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < R; ++k) s = fma(Ya[a][k], x[b * R + k], s);
        M[a][b] = s;
      }
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < R; ++k) s = fma(Ya[a][k], x[D * R + k], s);
      tt[a] = s - t0[a];
    }
    // columns of M, factored in place: col[b] = M[:, b] -> sigma_b u_b
    double col[D][D], V[D][D], nrm2[D], inv[D];
#pragma unroll
    for (int b = 0; b < D; ++b)
#pragma unroll
      for (int a = 0; a < D; ++a) col[b][a] = M[a][b];
    jacobi_columns<D, D>(col, V);
    jacobi_inv_norms<D, D>(col, nrm2, inv);
    int kmin = 0;
#pragma unroll
    for (int k = 1; k < D; ++k) kmin = (nrm2[k] < nrm2[kmin]) ? k : kmin;
#pragma unroll
    for (int k = 0; k < D; ++k)
#pragma unroll
      for (int a = 0; a < D; ++a) col[k][a] *= inv[k];
    double det;  // of U: +-1 up to round-off (0 when a column is numerically zero: nothing is flipped then)
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
    double* __restrict__ o = T + (size_t)i * B * D;
#pragma unroll
    for (int c = 0; c < D; ++c)
#pragma unroll
      for (int a = 0; a < D; ++a) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) s = fma(col[k][a], V[c][k], s);  // Rot(a, c) = sum_k u_k(a) V(c, k)
        o[c * D + a] = s;
      }
#pragma unroll
    for (int a = 0; a < D; ++a) o[D * D + a] = tt[a];
  }
}
