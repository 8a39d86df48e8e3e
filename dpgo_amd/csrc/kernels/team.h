// kernels/team.h -- the staircase step of a TEAM of agents on one device ("Team staircase"): the team's
// cost and Riemannian gradient in one launch, and the lift of the team vector to rank r + 1 along a witness with its
// retraction in one launch.  Part of kernels.h (included inside namespace dpgo, after certify.h: the member and tile tables
// are k_cert_apply_team's).
#pragma once

// ================================================================ f(X) and rgrad f(X) of the team, one launch
// X: the team vector [N, D+1, R] (member a owns the slice [first, first + n) in its internal pose order).  Rows of member a of
// X Q: X_a Q_aa + sum_b X_b Q_ba -- the own-row gather on the member's slice, then the coupling blocks of the row in slot
// order, each read straight from the other member's slice through nbr_pose (k_cert_apply_team's arithmetic and order): no
// neighbour buffer, no G, no exchange; the members' S, G and neighbour buffers are neither read nor written.  Then
// S_i = sym(Y_i^T (XQ)_rot,i) and rgrad_i = (XQ)_i - [Y_i S_i, 0] (k_grad's proj_col).
// partials[2 * blockIdx.x + {0, 1}]: sum <X_i, (XQ)_i> (f = half the total), sum |rgrad_i|^2 -- a fixed order inside the
// workgroup, k_cert_reduce sums the workgroups in a fixed order: bitwise the same run to run on one grid.
// WRG: the instance writes the rgrad tiles to RG [N, D+1, R] (team order); decided per instance, not by a per-lane branch.
template <int D, int R, bool WRG>
__global__ __launch_bounds__(kBlock) void k_team_eval(const CertMember* __restrict__ members,
                                                      const CertTile* __restrict__ tiles, int ntiles,
                                                      const double* __restrict__ X, double* __restrict__ RG,
                                                      double* __restrict__ partials) {
  using GEO = Geo<D, R, 1>;
  constexpr int B = GEO::B, T = GEO::T, BB = GEO::BB;
  __shared__ double sm[kWaves][2][GEO::G][GEO::T];
  __shared__ double red[kWaves * 2];
  const LaneId L = lane_id<D, 1>();
  double part[2] = {0.0, 0.0};
  const TileIter ti_ = tile_iter(ntiles);
  for (int tk = ti_.first; tk < ti_.last; tk += ti_.step) {
    const int mi = tiles[tk].member, p0 = tiles[tk].p0;
    const BsrDev Q = members[mi].Q, Cm = members[mi].C;
    const int32_t* __restrict__ nbr = members[mi].nbr_pose;
    const int first = members[mi].first, n = members[mi].n;
    const int il = p0 + L.wave * GEO::G + L.g;  // the member's pose
    const bool ok = (L.g < GEO::G) && (il < n);
    const int i = first + il;                   // the team's tile
    double eg[R], x[R];
    const size_t off = (size_t)i * T + L.c * R;
    double* ys = ok ? &sm[L.wave][0][L.g][0] : nullptr;
    double* ws = ok ? &sm[L.wave][1][L.g][0] : nullptr;
    q_gather<D, R, 1>(Q, X + (size_t)first * T, il, 0, L.c, ok, eg);
    if (ok) {
      const int t1 = Cm.rowptr[il + 1];
      for (int t = Cm.rowptr[il]; t < t1; ++t) {
        const double* __restrict__ q = Cm.vals + (size_t)t * BB + L.c * B;
        const double* __restrict__ xn = X + (size_t)nbr[Cm.colidx[t]] * T;
        double qk[B];
#pragma unroll
        for (int kk = 0; kk < B; ++kk) qk[kk] = q[kk];
#pragma unroll
        for (int kk = 0; kk < B; ++kk) {
#pragma unroll
          for (int a = 0; a < R; ++a) eg[a] = fma(xn[kk * R + a], qk[kk], eg[a]);
        }
      }
      load_col<R>(X + off, x);
#pragma unroll
      for (int a = 0; a < R; ++a) part[0] = fma(eg[a], x[a], part[0]);
      store_col<R>(ys + L.c * R, x);
      store_col<R>(ws + L.c * R, eg);
    }
    wave_sync();
    if (ok) {
      // proj_col's arithmetic without its branch on the column (which costs the R = D instances a private array in
      // scratch): the translation column gets s = 0 and keeps (XQ)_i
      double out[R], s[D];
      const int cr = L.c < D ? L.c : 0;
#pragma unroll
      for (int a = 0; a < D; ++a) {
        double p = 0.0, q = 0.0;
#pragma unroll
        for (int k = 0; k < R; ++k) {
          p = fma(ys[a * R + k], ws[cr * R + k], p);
          q = fma(ws[a * R + k], ys[cr * R + k], q);
        }
        s[a] = L.c < D ? 0.5 * (p + q) : 0.0;
      }
#pragma unroll
      for (int k = 0; k < R; ++k) {
        double v = eg[k];
#pragma unroll
        for (int a = 0; a < D; ++a) v = fma(-ys[a * R + k], s[a], v);
        out[k] = v;
      }
#pragma unroll
      for (int a = 0; a < R; ++a) part[1] = fma(out[a], out[a], part[1]);
      if constexpr (WRG) store_col<R>(RG + off, out);
    }
    wave_sync();
  }
  block_allreduce<2>(part, red);
  if (threadIdx.x == 0) {
    partials[(size_t)blockIdx.x * 2 + 0] = part[0];
    partials[(size_t)blockIdx.x * 2 + 1] = part[1];
  }
}

// ================================================================ X+ = qf([X; alpha w^T]): lift and retract, one launch
// X [n, D+1, R] -> X+ [n, D+1, R+1] along the witness w ((D+1) n doubles, one per tile column): the lifted tile is formed in
// the wave's LDS slot -- no lifted copy of X in memory -- and qf_col<D, R+1> maps its rotation columns onto the Stiefel
// manifold; the translation column is copied with its lifted entry.  Pose-wise: a team vector is one array of n = N poses.
// The arithmetic of k_cert_lift followed by k_retract<D, R+1> at scale 0, bit for bit.
template <int D, int R>
__global__ __launch_bounds__(kBlock) void k_cert_lift_retract(const double* __restrict__ X, const double* __restrict__ w,
                                                              double alpha, double* __restrict__ X2, int n) {
  using GEO = Geo<D, R + 1>;
  constexpr int R1 = R + 1;
  __shared__ double sm[kWaves][GEO::G][GEO::T];
  const LaneId L = lane_id<D>();
  const int ntiles = (n + GEO::P - 1) / GEO::P;
  const TileIter ti_ = tile_iter(ntiles);
  for (int tile = ti_.first; tile < ti_.last; tile += ti_.step) {
    const int i = tile * GEO::P + L.wave * GEO::G + L.g;
    const bool ok = (L.g < GEO::G) && (i < n);
    const size_t col = (size_t)i * GEO::B + L.c;
    double* as = ok ? &sm[L.wave][L.g][0] : nullptr;
    double a[R1];
    if (ok) {
      double x[R];
      load_col<R>(X + col * R, x);
#pragma unroll
      for (int k = 0; k < R; ++k) a[k] = x[k];
      a[R] = alpha * w[col];
      store_col<R1>(as + L.c * R1, a);
    }
    wave_sync();
    if (ok) {
      qf_col<D, R1>(as, L.c, a);
      store_col<R1>(X2 + col * R1, a);
    }
    wave_sync();
  }
}
