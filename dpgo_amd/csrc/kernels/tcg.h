// kernels/tcg.h -- the two kernels of the tCG loop (fused Hessian step and residual / iterate update): shared scalar prologues,
// the generic-layout kernels (odd tile size) and the span kernels (even tile size: every 3-D case).
// Part of kernels.h (included inside namespace dpgo, in this order: common.h, problem.h, tcg.h, persist.h, multilevel.h, dense.h, manifold.h, rtr.h, agent.h, init.h).
#pragma once

// ================================================================ K7b + K1/K3/K2 fused: one tCG step
// One launch per tCG iteration:
//  (i)   prologue = the scalar half of the direction update (ROPTLIB tCG_TR): convergence test
//        |r| <= |r0| min(|r0|^theta, kappa), beta = z_r'/z_r, e_Pd / d_Pd recurrences, from the
//        <r,r>, <z,r> partials of k_tcg_update (first = 1: norm_r0, z_r, d_Pd initialisation);
//  (ii)  Hz = proj_X( z Q - z_rot S ): the block-SpMM gathers the preconditioned residual z;
//  (iii) row-local, in place:  delta <- beta*delta - z,   H delta <- beta*(H delta) - Hz
//        (H is linear on the tangent space, so this equals H applied to the new delta; it lets the
//        direction update ride in the SpMM epilogue instead of costing a second gather or a separate
//        kernel: 3 -> 2 launches per tCG iteration), and the <delta, H delta> partial.
// The oracle has the same option (hess_recurrence) for trajectory-level parity tests.
// ---------------------------------------------------------------- tCG scalar prologues (shared)
// Direction-update scalars (ROPTLIB tCG_TR): returns false when this launch has nothing left to do.
__device__ __forceinline__ bool tcg_hess_prologue(DevState& st, const double* __restrict__ pin, int nb_in, int first,
                                                  double* red, double& beta, const PartialRaw<2>* early = nullptr) {
  double pr[2];
  if (early)
    partials_finish<2>(*early, pr, red);
  else
    load_partials<2>(pin, nb_in, pr, red);
  const double r_r = pr[0], z_r_new = pr[1];
  beta = 0.0;
  if (first) {
    st.norm_r0 = sqrt(r_r);
    st.z_r = z_r_new;
    st.d_Pd = z_r_new;
    st.e_Pd = 0.0;
    if (st.max_inner <= 0) {
      st.tcg_done = 1;
      return false;
    }
    return true;
  }
  const double norm_r = sqrt(r_r);
  const double pw = (st.theta == 1.0) ? st.norm_r0 : pow(st.norm_r0, st.theta);  // theta = 1 (reference default)
  if (st.tcg_j >= st.min_inner && norm_r <= st.norm_r0 * (pw < st.kappa ? pw : st.kappa)) {
    st.tcg_status = (st.kappa < pw) ? TCG_LCON : TCG_SCON;
    st.tcg_done = 1;
    return false;
  }
  beta = z_r_new / st.z_r;
  st.e_Pd = beta * (st.e_Pd + st.alpha * st.d_Pd);
  st.d_Pd = z_r_new + beta * beta * st.d_Pd;
  st.z_r = z_r_new;
  st.tcg_j += 1;
  if (st.tcg_j >= st.max_inner) {
    st.tcg_done = 1;
    st.tcg_status = TCG_MAXITER;
    return false;
  }
  return true;
}

// Step-length scalars: mode 0 = normal step, 1 = boundary step (eta += tau*delta, stop), 2 = initialisation.
__device__ __forceinline__ int tcg_update_prologue(DevState& st, const double* __restrict__ pin, int nb_in, int first,
                                                   double* red, double& alpha, double& tau,
                                                   const PartialRaw<1>* early = nullptr) {
  alpha = 0.0;
  tau = 0.0;
  if (first) {
    st.tcg_done = 0;
    st.tcg_j = 0;
    st.tcg_status = TCG_MAXITER;
    st.e_Pe = 0.0;
    st.e_Pd = 0.0;
    return 2;
  }
  double dh[1];
  if (early)
    partials_finish<1>(*early, dh, red);
  else
    load_partials<1>(pin, nb_in, dh, red);
  const double d_Hd = dh[0];
  alpha = st.z_r / d_Hd;
  const double e_Pe_new = st.e_Pe + 2.0 * alpha * st.e_Pd + alpha * alpha * st.d_Pd;
  st.n_hess += 1;
  st.alpha = alpha;
  const double D2 = st.Delta * st.Delta;
  if (d_Hd <= 0.0 || e_Pe_new >= D2) {
    tau = (-st.e_Pd + sqrt(st.e_Pd * st.e_Pd + st.d_Pd * (D2 - st.e_Pe))) / st.d_Pd;
    st.tcg_status = (d_Hd < 0.0) ? TCG_NEGCURV : TCG_EXCREGION;
    st.tcg_done = 1;
    return 1;
  }
  st.e_Pe = e_Pe_new;
  return 0;
}

// ---------------------------------------------------------------- kept directions (DEF = 1)
// Nothing inside a tCG run reads the iterate eta: the trust-region norms come from the scalar recurrences above and the rho
// test reads eta once, in k_retract.  A solve whose direction ring fits (host: tcg_dirs_ensure) therefore keeps the
// directions instead of summing them every iteration:
//  * the Hessian-step kernels read delta_{k-1} from slot k-1 of the ring and write delta_k to slot k (`delta` is the ring,
//    a slot is n * T doubles), k = the iteration index the prologue has just computed (0 with `first`, else st.tcg_j): the
//    same bytes as the in-place update, and a launch that exits early touches nothing.  k < max_inner <= slots of the ring;
//  * the update kernels load neither delta nor eta and store no eta; the thread that stores the state record also stores
//    this iteration's step length (alpha, or tau on the boundary step) and the number of steps so far into `coef`:
//    coef[0] = count (0 from the initialisation), coef[1 + j] = step length of iteration j;
//  * k_retract folds eta = fma(c_{K-1}, delta_{K-1}, ... fma(c_0, delta_0, +0)) while it loads its tile: the same fused
//    multiply-adds in the same order on the same operands as the running sum, so every bit of eta is the same.
template <int DEF>
__device__ __forceinline__ void tcg_store_coef(double* __restrict__ coef, const DevState& st, int mode, double alpha, double tau) {
  if constexpr (DEF) {
    if (mode == 2) {
      coef[0] = 0.0;
    } else {
      coef[1 + st.tcg_j] = (mode == 1) ? tau : alpha;
      coef[0] = (double)(st.tcg_j + 1);
    }
  }
}

template <int D, int R, int SPLIT, int DEF = 0>
__global__ __launch_bounds__(kBlock, DPGO_LB_HESS) void k_tcg_hess(BsrDev Q, const double* __restrict__ X,
                                                     const double* __restrict__ S, const double* __restrict__ z,
                                                     double* __restrict__ delta, double* __restrict__ Hd,
                                                     const double* __restrict__ pin, int nb_in,
                                                     double* __restrict__ pout, const DevState* __restrict__ sin,
                                                     DevState* __restrict__ sout, int first, int n,
                                                     unsigned long long* hflag, unsigned gen) {
  // generic layout (odd tile size: the 2-D cases with odd r); even tile sizes run k_tcg_hess_span
  using GEO = Geo<D, R, SPLIT>;
  __shared__ __attribute__((aligned(16))) double sm[kWaves][3][GEO::G][GEO::T];
  __shared__ double red[kWaves * kNP];
  DevState st;
  load_state(st, sin);
  gen = state_gen(st, gen);
  if (st.rtr_stop || st.tcg_done) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      store_state(sout, st);
      publish_progress(hflag, gen, st);
    }
    return;
  }
  double beta;
  const bool go = tcg_hess_prologue(st, pin, nb_in, first, red, beta);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    store_state(sout, st);
    publish_progress(hflag, gen, st);
  }
  if (!go) return;
  // (DEF: slot k of the ring receives delta_k, slot k - 1 holds delta_{k-1})
  double* dout = delta;
  if constexpr (DEF) dout = delta + (size_t)(first ? 0 : st.tcg_j) * ((size_t)n * GEO::T);
  const double* din = (DEF && !first) ? dout - (size_t)n * GEO::T : dout;

  const LaneId L = lane_id<D, SPLIT>();
  const int ntiles = (n + GEO::P - 1) / GEO::P;
  double part[1] = {0.0};
  const TileIter ti_ = tile_iter(ntiles);
  for (int tile = ti_.first; tile < ti_.last; tile += ti_.step) {
    const int i = tile * GEO::P + L.wave * GEO::G + L.g;
    const bool okp = (L.g < GEO::G) && (i < n);
    const bool ok = okp && (L.s == 0);
    double h[R], zc[R], x[R];
    const size_t off = (size_t)i * GEO::T + L.c * R;
    double* ys = ok ? &sm[L.wave][0][L.g][0] : nullptr;
    double* vs = ok ? &sm[L.wave][1][L.g][0] : nullptr;
    double* hs = ok ? &sm[L.wave][2][L.g][0] : nullptr;
    // issue the epilogue's loads first: they overlap the gather's index -> tile latency chain
    double srow[D], dl[R], hd[R];
    if (ok) {
      load_col<R>(X + off, x);
      load_col<R>(z + off, zc);
      if (L.c < D) {
#pragma unroll
        for (int a = 0; a < D; ++a) srow[a] = S[(size_t)i * D * D + L.c * D + a];
      }
      if (!first) {
        load_col<R>(din + off, dl);
        load_col<R>(Hd + off, hd);
      }
    }
    spmm_col<D, R, SPLIT>(Q.rowptr, Q.colidx, Q.vals, z, i, L.s, L.c, okp, h);
    if (ok) {
      store_col<R>(ys + L.c * R, x);
      store_col<R>(vs + L.c * R, zc);
    }
    wave_sync();
    if (ok) {
      if (L.c < D) {
#pragma unroll
        for (int a = 0; a < D; ++a) {
#pragma unroll
          for (int k = 0; k < R; ++k) h[k] = fma(-vs[a * R + k], srow[a], h[k]);
        }
      }
      store_col<R>(hs + L.c * R, h);
    }
    wave_sync();
    if (ok) {
      double hz[R], s[D];
      proj_col<D, R>(ys, hs, L.c, h, hz, s);
      if (first) {
#pragma unroll
        for (int a = 0; a < R; ++a) {
          dl[a] = -zc[a];
          hd[a] = -hz[a];
        }
      } else {
#pragma unroll
        for (int a = 0; a < R; ++a) {
          dl[a] = fma(beta, dl[a], -zc[a]);
          hd[a] = fma(beta, hd[a], -hz[a]);
        }
      }
#pragma unroll
      for (int a = 0; a < R; ++a) part[0] = fma(dl[a], hd[a], part[0]);
      store_col<R>(dout + off, dl);
      store_col<R>(Hd + off, hd);
    }
    wave_sync();
  }
  store_partials<1>(part, pout, red);
}

// ================================================================ span kernels (pose tile size even: all 3-D cases)
// Same arithmetic as k_tcg_hess / k_tcg_update; the differences are purely about memory:
//  * own-tile vectors move as lane-linear 16-byte pieces (Span<>), element-wise recurrences run in span layout;
//  * the FIRST tile's global loads (row pointer, column indices, vector pieces) are issued before the scalar
//    prologue (state record + partial-sum reduction), so the two dependent-latency chains overlap -- this is
//    what matters for small blocks (multi-GPU strong scaling), where a kernel is a chain of ~15 memory latencies.
template <int D, int R, int SPLIT, int NTS = 0, int DEF = 0>
__global__ __launch_bounds__(kBlock) void k_tcg_hess_span(BsrDev Q, const double* __restrict__ X,
                                                          const double* __restrict__ S, const double* __restrict__ z,
                                                          double* __restrict__ delta, double* __restrict__ Hd,
                                                          const double* __restrict__ pin, int nb_in,
                                                          double* __restrict__ pout, const DevState* __restrict__ sin,
                                                          DevState* __restrict__ sout, int first, int n,
                                                          unsigned long long* hflag, unsigned gen) {
  using GEO = Geo<D, R, SPLIT>;
  using SPN = Span<D, R, SPLIT>;
  __shared__ __attribute__((aligned(16))) double sm[kWaves][4][GEO::G][GEO::T];
  __shared__ double red[kWaves * kNP];
  const LaneId L = lane_id<D, SPLIT>();
  const int lane = threadIdx.x & 63;
  const int ntiles = (n + GEO::P - 1) / GEO::P;
  const TileIter ti_ = tile_iter(ntiles);
  double* ys = &sm[L.wave][0][0][0];
  double* vs = &sm[L.wave][1][0][0];
  double* hs = &sm[L.wave][2][0][0];
  double* os = &sm[L.wave][3][0][0];

  // ---- per-tile prefetch state
  RowIdx ri;
  dbl2 xv[SPN::NIT], zv[SPN::NIT], dv[SPN::NIT], hv[SPN::NIT];
  double srow[D];
  int p0 = 0, valid = 0, i = 0;
  bool okp = false, ok = false;
  // (DEF: the ring slots this launch reads and writes follow from the prologue: the first tile's piece of delta_{k-1} is
  // requested behind it -- an early-exit launch must not touch the ring, its tcg_j may equal the number of slots)
  const double* din = DEF ? nullptr : delta;
  double* dout = delta;
  auto prefetch = [&](int tile) {
    p0 = tile * GEO::P + L.wave * GEO::G;
    const int npose = (n - p0) < GEO::G ? (n - p0) : GEO::G;
    valid = npose > 0 ? npose * GEO::T : 0;
    i = p0 + L.g;
    okp = (L.g < GEO::G) && (i < n);
    ok = okp && (L.s == 0);
    ri = row_idx_load<D, SPLIT>(Q.rowptr, Q.colidx, i, L.s, L.c, okp);
    const size_t base = (size_t)p0 * GEO::T;
    const dbl2* X2 = reinterpret_cast<const dbl2*>(X + base);
    const dbl2* z2 = reinterpret_cast<const dbl2*>(z + base);
    const dbl2* h2 = reinterpret_cast<const dbl2*>(Hd + base);
#pragma unroll
    for (int it = 0; it < SPN::NIT; ++it) {
      const int pc = lane + 64 * it;
      if (2 * pc < valid) {
        xv[it] = ld_stream<NTS>(X2 + pc);
        zv[it] = z2[pc];
        if (!first) {
          if (!DEF || din) dv[it] = ld_stream<NTS>(reinterpret_cast<const dbl2*>(din + base) + pc);
          hv[it] = ld_stream<NTS>(h2 + pc);
        }
      }
    }
    if (ok && L.c < D) {
#pragma unroll
      for (int a = 0; a < D; ++a) srow[a] = ld_stream<NTS>(S + (size_t)i * D * D + L.c * D + a);
    }
  };
  // ---- everything the prologue needs is requested before the first wait: state record (scalar loads), the
  // previous kernel's partial sums (small blocks only: the registers would cost the big-block kernel an
  // occupancy step), then the first tile.  A small-block launch is a chain of dependent memory round trips
  // (rocprof: 9.4 us for 2500 poses); this takes two of them off the chain.
  DPGO_TL_DECL;
  DPGO_STAMP(0, 0);
  DevState st;
  load_state(st, sin);
  gen = state_gen(st, gen);
  [[maybe_unused]] PartialRaw<2> praw;
  if constexpr (SPLIT > 1) partials_issue<2>(pin, nb_in, praw);
  int tile = ti_.first;
  bool have = tile < ti_.last;
  if (have) prefetch(tile);

  DPGO_STAMP(0, 1);
  // ---- scalar prologue
  if (st.rtr_stop || st.tcg_done) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      store_state(sout, st);
      publish_progress(hflag, gen, st);
    }
    return;
  }
  double beta;
  const bool go = tcg_hess_prologue(st, pin, nb_in, first, red, beta, (SPLIT > 1) ? &praw : nullptr);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    store_state(sout, st);
    publish_progress(hflag, gen, st);
  }
  if (!go) return;
  DPGO_STAMP(0, 2);
  if constexpr (DEF) {
    dout = delta + (size_t)(first ? 0 : st.tcg_j) * ((size_t)n * GEO::T);
    if (!first) {
      din = dout - (size_t)n * GEO::T;
      if (have) {
        const dbl2* d2 = reinterpret_cast<const dbl2*>(din + (size_t)p0 * GEO::T);
#pragma unroll
        for (int it = 0; it < SPN::NIT; ++it) {
          const int pc = lane + 64 * it;
          if (2 * pc < valid) dv[it] = ld_stream<NTS>(d2 + pc);
        }
      }
    }
  }

  double part[1] = {0.0};
  while (have) {
#pragma unroll
    for (int it = 0; it < SPN::NIT; ++it) {
      const int pc = lane + 64 * it;
      if (2 * pc < valid) {
        reinterpret_cast<dbl2*>(ys)[pc] = xv[it];
        reinterpret_cast<dbl2*>(vs)[pc] = zv[it];
      }
    }
    DPGO_STAMP(0, 3);
    double h[R];
    spmm_col_pre<D, R, SPLIT>(ri, Q.colidx, Q.vals, z, L.s, L.c, h);
    wave_sync();
    DPGO_STAMP(0, 4);
    if (ok) {
      if (L.c < D) {
        const double* vt = vs + L.g * GEO::T;
#pragma unroll
        for (int a = 0; a < D; ++a) {
#pragma unroll
          for (int k = 0; k < R; ++k) h[k] = fma(-vt[a * R + k], srow[a], h[k]);
        }
      }
      store_col<R>(hs + L.g * GEO::T + L.c * R, h);
    }
    wave_sync();
    if (ok) {
      double hz[R], sdummy[D];
      proj_col<D, R>(ys + L.g * GEO::T, hs + L.g * GEO::T, L.c, h, hz, sdummy);
      store_col<R>(os + L.g * GEO::T + L.c * R, hz);
    }
    wave_sync();
    {
      const size_t base = (size_t)p0 * GEO::T;
      dbl2* d2 = reinterpret_cast<dbl2*>(dout + base);
      dbl2* h2 = reinterpret_cast<dbl2*>(Hd + base);
#pragma unroll
      for (int it = 0; it < SPN::NIT; ++it) {
        const int pc = lane + 64 * it;
        if (2 * pc < valid) {
          const dbl2 hzv = reinterpret_cast<const dbl2*>(os)[pc];
          dbl2 dn, hn;
          if (first) {
            dn.x = -zv[it].x;
            dn.y = -zv[it].y;
            hn.x = -hzv.x;
            hn.y = -hzv.y;
          } else {
            dn.x = fma(beta, dv[it].x, -zv[it].x);
            dn.y = fma(beta, dv[it].y, -zv[it].y);
            hn.x = fma(beta, hv[it].x, -hzv.x);
            hn.y = fma(beta, hv[it].y, -hzv.y);
          }
          st_stream<NTS>(d2 + pc, dn);
          st_stream<NTS>(h2 + pc, hn);
          part[0] = fma(dn.x, hn.x, part[0]);
          part[0] = fma(dn.y, hn.y, part[0]);
        }
      }
    }
    wave_sync();
    DPGO_STAMP(0, 5);
    tile += ti_.step;
    have = tile < ti_.last;
    if (have) prefetch(tile);
  }
  store_partials<1>(part, pout, red);
  DPGO_STAMP(0, 6);
  DPGO_COMMIT(0);
}

// k_tcg_hess_span on the symmetric storage of Q (spmm_sym_pre, common.h): big blocks only (one pose per D+1 lanes).  The
// own-tile pieces of delta / H delta are requested after the gather instead of one tile ahead and z is re-read from LDS
// (registers).  The gather keeps the loads of DPGO_HESS_BATCH blocks in flight per wave, which costs the third wave per SIMD
// (217 VGPRs) and still wins: 2 waves x 4 blocks in flight against 3 x 1 (39.7 -> 37.3 us).  In-kernel timeline of a tile
// (tools/timeline_tiles.py, profiles/r05_v4_timeline_tiles.txt): ~8 us, of which the gather's two round trips 3 us and the
// epilogue behind it 4 us.  Tried on top and measured neutral, i.e. the launch is bound by what the memory system
// delivers to 512 resident workgroups, not by one wave's chain of round trips: delta / H delta requested in front of the
// gather (37.4..37.7 us), a three-stage pipeline over the tiles (row extents two tiles ahead, indices + own X, z, S one tile
// ahead: tile 7 us, launch 37.4..38.0 us), the previous kernel's partial sums requested in front of the first tile.
template <int D, int R, int NTS, int DEF = 0>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(DPGO_SYM_WAVES, DPGO_SYM_WAVES))) void k_tcg_hess_sym(BsrSymDev Q, const double* __restrict__ X,
                                                          const double* __restrict__ S, const double* __restrict__ z,
                                                          double* __restrict__ delta, double* __restrict__ Hd,
                                                          const double* __restrict__ pin, int nb_in,
                                                          double* __restrict__ pout, const DevState* __restrict__ sin,
                                                          DevState* __restrict__ sout, int first, int n,
                                                          unsigned long long* hflag, unsigned gen) {
  constexpr int SPLIT = 1;
  using GEO = Geo<D, R, SPLIT>;
  using SPN = Span<D, R, SPLIT>;
  __shared__ __attribute__((aligned(16))) double sm[kWaves][4][GEO::G][GEO::T];
  __shared__ double red[kWaves * kNP];
  const LaneId L = lane_id<D, SPLIT>();
  const int lane = threadIdx.x & 63;
  const int ntiles = (n + GEO::P - 1) / GEO::P;
  const TileIter ti_ = tile_iter(ntiles);
  double* ys = &sm[L.wave][0][0][0];
  double* vs = &sm[L.wave][1][0][0];
  double* hs = &sm[L.wave][2][0][0];
  double* os = &sm[L.wave][3][0][0];

  // ---- per-tile prefetch state
  SymIdx si;
  dbl2 xv[SPN::NIT], zv[SPN::NIT];
  double srow[D];
  int p0 = 0, valid = 0, i = 0;
  bool okp = false, ok = false;
  auto prefetch = [&](int tk) {
    const int tile = tile_of(Q, tk);  // (the walk over the tiles: BsrSymDevT::tord)
    p0 = tile * GEO::P + L.wave * GEO::G;
    const int npose = (n - p0) < GEO::G ? (n - p0) : GEO::G;
    valid = npose > 0 ? npose * GEO::T : 0;
    i = p0 + L.g;
    okp = (L.g < GEO::G) && (i < n);
    ok = okp && (L.s == 0);
    si = sym_idx_load<D>(Q, i, L.c, okp);
    const size_t base = (size_t)p0 * GEO::T;
    const dbl2* X2 = reinterpret_cast<const dbl2*>(X + base);
    const dbl2* z2 = reinterpret_cast<const dbl2*>(z + base);
#pragma unroll
    for (int it = 0; it < SPN::NIT; ++it) {
      const int pc = lane + 64 * it;
      if (2 * pc < valid) {
        xv[it] = ld_stream<NTS>(X2 + pc);
        zv[it] = z2[pc];
      }
    }
    if (ok && L.c < D) {
#pragma unroll
      for (int a = 0; a < D; ++a) srow[a] = ld_stream<NTS>(S + (size_t)i * D * D + L.c * D + a);
    }
  };
  // ---- everything the prologue needs is requested before the first wait: state record (scalar loads), the
  // previous kernel's partial sums (small blocks only: the registers would cost the big-block kernel an
  // occupancy step), then the first tile.  A small-block launch is a chain of dependent memory round trips
  // (rocprof: 9.4 us for 2500 poses); this takes two of them off the chain.
  DPGO_TL_DECL;
  DPGO_TL_TILES_DECL;
  DPGO_STAMP(0, 0);
  DevState st;
  load_state(st, sin);
  gen = state_gen(st, gen);
  [[maybe_unused]] PartialRaw<2> praw;
  int tile = ti_.first;
  bool have = tile < ti_.last;
  if (have) prefetch(tile);

  DPGO_STAMP(0, 1);
  // ---- scalar prologue
  if (st.rtr_stop || st.tcg_done) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      store_state(sout, st);
      publish_progress(hflag, gen, st);
    }
    return;
  }
  double beta;
  const bool go = tcg_hess_prologue(st, pin, nb_in, first, red, beta, (SPLIT > 1) ? &praw : nullptr);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    store_state(sout, st);
    publish_progress(hflag, gen, st);
  }
  if (!go) return;
  // (DEF: slot k of the ring receives delta_k, slot k - 1 holds delta_{k-1})
  double* dout = delta;
  if constexpr (DEF) dout = delta + (size_t)(first ? 0 : st.tcg_j) * ((size_t)n * GEO::T);
  const double* din = (DEF && !first) ? dout - (size_t)n * GEO::T : dout;
  DPGO_STAMP(0, 2);
  DPGO_STAMP_ENTRY;
  DPGO_STAMP_AT(1);

  double part[1] = {0.0};
  while (have) {
    DPGO_STAMP_TILE(0);
#pragma unroll
    for (int it = 0; it < SPN::NIT; ++it) {
      const int pc = lane + 64 * it;
      if (2 * pc < valid) {
        reinterpret_cast<dbl2*>(ys)[pc] = xv[it];
        reinterpret_cast<dbl2*>(vs)[pc] = zv[it];
      }
    }
    DPGO_STAMP(0, 3);
    DPGO_STAMP_TILE(1);
    double h[R];
    spmm_sym_pre<D, R, DPGO_HESS_BATCH>(si, Q, z, L.c, h);
    DPGO_TL_USE(h[0]);
    DPGO_STAMP_TILE(2);
    // delta, H delta of the own tile: requested after the gather (its accumulators need the registers), consumed after
    // the projection
    dbl2 dv[SPN::NIT], hv[SPN::NIT];
    if (!first) {
      const size_t base = (size_t)p0 * GEO::T;
      const dbl2* d2 = reinterpret_cast<const dbl2*>(din + base);
      const dbl2* h2 = reinterpret_cast<const dbl2*>(Hd + base);
#pragma unroll
      for (int it = 0; it < SPN::NIT; ++it) {
        const int pc = lane + 64 * it;
        if (2 * pc < valid) {
          dv[it] = ld_stream<NTS>(d2 + pc);
          hv[it] = ld_stream<NTS>(h2 + pc);
        }
      }
    }
    wave_sync();
    DPGO_STAMP(0, 4);
    DPGO_STAMP_TILE(3);
    if (ok) {
      if (L.c < D) {
        const double* vt = vs + L.g * GEO::T;
#pragma unroll
        for (int a = 0; a < D; ++a) {
#pragma unroll
          for (int k = 0; k < R; ++k) h[k] = fma(-vt[a * R + k], srow[a], h[k]);
        }
      }
      store_col<R>(hs + L.g * GEO::T + L.c * R, h);
    }
    wave_sync();
    if (ok) {
      double hz[R], sdummy[D];
      proj_col<D, R>(ys + L.g * GEO::T, hs + L.g * GEO::T, L.c, h, hz, sdummy);
      store_col<R>(os + L.g * GEO::T + L.c * R, hz);
    }
    wave_sync();
    DPGO_STAMP_TILE(4);
    {
      const size_t base = (size_t)p0 * GEO::T;
      dbl2* d2 = reinterpret_cast<dbl2*>(dout + base);
      dbl2* h2 = reinterpret_cast<dbl2*>(Hd + base);
#pragma unroll
      for (int it = 0; it < SPN::NIT; ++it) {
        const int pc = lane + 64 * it;
        if (2 * pc < valid) {
          const dbl2 hzv = reinterpret_cast<const dbl2*>(os)[pc];
          const dbl2 zl = reinterpret_cast<const dbl2*>(vs)[pc];
          dbl2 dn, hn;
          if (first) {
            dn.x = -zl.x;
            dn.y = -zl.y;
            hn.x = -hzv.x;
            hn.y = -hzv.y;
          } else {
            dn.x = fma(beta, dv[it].x, -zl.x);
            dn.y = fma(beta, dv[it].y, -zl.y);
            hn.x = fma(beta, hv[it].x, -hzv.x);
            hn.y = fma(beta, hv[it].y, -hzv.y);
          }
          st_stream<NTS>(d2 + pc, dn);
          st_stream<NTS>(h2 + pc, hn);
          part[0] = fma(dn.x, hn.x, part[0]);
          part[0] = fma(dn.y, hn.y, part[0]);
        }
      }
    }
    wave_sync();
    DPGO_STAMP(0, 5);
    tile += ti_.step;
    have = tile < ti_.last;
    if (have) prefetch(tile);
    DPGO_STAMP_TILE(5);
    DPGO_TILE_NEXT;
  }
  store_partials<1>(part, pout, red);
  DPGO_STAMP(0, 6);
  DPGO_STAMP_AT(2);
  DPGO_COMMIT(0);
}

#ifndef DPGO_UPDATE_WAVES
#define DPGO_UPDATE_WAVES 0  // waves per SIMD k_tcg_update_span is compiled for (0: the compiler's choice -- 203 VGPRs = 2 waves)
#endif
// ML = 1: the launch is known to be in multilevel mode (ml_omega > 0: z receives the unprojected pre-smoothing step, the
// iterate is not read) -- the instance the 100k loop launches: without the iterate's pieces and the projection it fits
// DPGO_UPDATE_WAVES_ML waves per SIMD.  ML = 0: the mode is the runtime argument (block-Jacobi / no preconditioner / either).
#ifndef DPGO_UPDATE_WAVES_ML
#define DPGO_UPDATE_WAVES_ML 3
#endif
// DEF = 1 (kept directions, see above k_tcg_hess): delta and eta are not touched (null), the step length goes to `coef`.
// (3, 5): the multilevel instance drops from 147 to 119 VGPRs; it stays at DPGO_UPDATE_WAVES_ML waves -- a fourth workgroup
// per CU does not fit the LDS (4 x 41 088 bytes), and the grid, hence the order of the partial sums, is the reference's.
// PIPE = 1 (DPGO_UPDATE_PIPE, the default; 0 = the reference order, same bits): the next tile is requested while this one is
// still being finished, see request_next below.  It costs the registers of a second tile's geometry and block-Jacobi row
// and whatever the compiler then keeps live: (3, 5) DEF = 1 goes from 119 to 157 VGPRs, still three waves, no scratch.  The
// instances that do not hold their occupancy that way have no PIPE = 1 form (kUpdatePipe: the launch picks PIPE = 0):
//  * ML = 1, DEF = 0 at 20 and more doubles per pose, (3, 5) and (3, 6): four piece sets (eta, delta, H delta, r) in flight
//    need 168 VGPRs and 180 / 232 bytes of scratch per lane; up to 16 doubles per pose it fits (115-164 VGPRs);
//  * every ML = 0 instance: (3, 5) goes from 209 VGPRs to 256 + 20 AGPRs (2 -> 1 wave), (3, 3) DEF = 1 from 4 waves to 2.
template <int D, int R, int DEF>
constexpr int kUpdatePipe = (DEF || Geo<D, R>::T <= 16) ? 1 : 0;
template <int D, int R, int ML = 0, int DEF = 0, int PIPE = 0>
__global__ __launch_bounds__(kBlock)
    __attribute__((amdgpu_waves_per_eu(ML ? DPGO_UPDATE_WAVES_ML : (DPGO_UPDATE_WAVES ? DPGO_UPDATE_WAVES : 1),
                                       ML ? DPGO_UPDATE_WAVES_ML : (DPGO_UPDATE_WAVES ? DPGO_UPDATE_WAVES : 8))))
void k_tcg_update_span(const double* __restrict__ X, const double* __restrict__ g,
                                                            const double* __restrict__ dinv,
                                                            const double* __restrict__ delta,
                                                            const double* __restrict__ Hd, double* __restrict__ eta,
                                                            double* __restrict__ r, double* __restrict__ z,
                                                            const double* __restrict__ pin, int nb_in,
                                                            double* __restrict__ pout, const DevState* __restrict__ sin,
                                                            DevState* __restrict__ sout, int first, int n,
                                                            unsigned long long* hflag, unsigned gen,
                                                            double ml_omega, double* __restrict__ coef,
                                                            float* __restrict__ z32 = nullptr) {
  // ml_omega > 0 (fused multilevel preconditioner): z receives the pre-smoothing step w Dinv r, unprojected -- into z32
  // instead, rounded to fp32, when the cycle keeps its internal vectors in that storage (kernel-uniform)
  using GEO = Geo<D, R>;
  using SPN = Span<D, R, 1>;
  __shared__ __attribute__((aligned(16))) double sm[kWaves][4][GEO::G][GEO::T];
  __shared__ double red[kWaves * kNP];
  const LaneId L = lane_id<D>();
  const int lane = threadIdx.x & 63;
  const int ntiles = (n + GEO::P - 1) / GEO::P;
  const TileIter ti_ = tile_iter(ntiles);
  double* ys = &sm[L.wave][0][0][0];
  double* rs = &sm[L.wave][1][0][0];
  double* zs = &sm[L.wave][2][0][0];
  double* os = &sm[L.wave][3][0][0];

  const bool ml_mode = ML ? true : (ml_omega > 0.0);  // (ML: compile-time)
  dbl2 xv[SPN::NIT], ev[SPN::NIT], dv[SPN::NIT], hv[SPN::NIT], rv[SPN::NIT];
  double drow[GEO::B];
  int p0 = 0, valid = 0, i = 0;
  bool ok = false;
  // (PIPE: the geometry and the block-Jacobi row of the tile in flight, beside the ones of the tile being finished)
  [[maybe_unused]] double drow_n[GEO::B];
  [[maybe_unused]] int p0_n = 0, valid_n = 0, i_n = 0;
  [[maybe_unused]] bool ok_n = false;
  auto request = [&](int tile, int& p0_, int& valid_, int& i_, bool& ok_, double (&drow_)[GEO::B]) {
    p0_ = tile * GEO::P + L.wave * GEO::G;
    const int npose = (n - p0_) < GEO::G ? (n - p0_) : GEO::G;
    valid_ = npose > 0 ? npose * GEO::T : 0;
    i_ = p0_ + L.g;
    ok_ = (L.g < GEO::G) && (i_ < n);
    const size_t base = (size_t)p0_ * GEO::T;
    const dbl2* X2 = reinterpret_cast<const dbl2*>(X + base);
    const dbl2* g2 = reinterpret_cast<const dbl2*>(g + base);
    [[maybe_unused]] const dbl2* e2 = reinterpret_cast<const dbl2*>(eta + base);
    [[maybe_unused]] const dbl2* d2 = reinterpret_cast<const dbl2*>(delta + base);
    const dbl2* h2 = reinterpret_cast<const dbl2*>(Hd + base);
    const dbl2* r2 = reinterpret_cast<const dbl2*>(r + base);
#pragma unroll
    for (int it = 0; it < SPN::NIT; ++it) {
      const int pc = lane + 64 * it;
      if (2 * pc < valid_) {
        // (the iterate is only needed by the tangent projection of the block-Jacobi / unpreconditioned z; the multilevel
        // pre-smoothing step x1 = w Dinv r is not projected: 16 MB less per launch at 100k poses)
        if (!ml_mode) xv[it] = X2[pc];
        if (first) {
          rv[it] = g2[pc];
        } else {
          if constexpr (!DEF) {
            ev[it] = e2[pc];
            dv[it] = d2[pc];
          }
          hv[it] = h2[pc];
          rv[it] = r2[pc];
        }
      }
    }
    if (ok_ && dinv) {
#pragma unroll
      for (int k = 0; k < GEO::B; ++k) drow_[k] = dinv[(size_t)i_ * GEO::BB + L.c * GEO::B + k];
    }
  };
  auto prefetch = [&](int tile) { request(tile, p0, valid, i, ok, drow); };
  // PIPE = 1: the next tile is requested as soon as the piece registers of this one are consumed -- behind the first
  // per-piece loop, which is the last reader of xv / ev / dv / hv / rv -- so its round trip runs under the block-Jacobi
  // step, the LDS passes and the stores of z instead of starting behind them.  The pieces it loads are other addresses
  // than the ones just stored; the arithmetic, its order and every store are those of PIPE = 0 (DPGO_UPDATE_PIPE=0).
  auto request_next = [&](int& tile, bool& have) {
    if constexpr (PIPE) {
      tile += ti_.step;
      have = tile < ti_.last;
      if (have) request(tile, p0_n, valid_n, i_n, ok_n, drow_n);
    }
  };
  DPGO_TL_DECL;
  DPGO_STAMP(1, 0);
  // state record and partial sums are requested before the first tile (see k_tcg_hess_span)
  DevState st;
  load_state(st, sin);
  gen = state_gen(st, gen);
  PartialRaw<1> praw;
  partials_issue<1>(pin, nb_in, praw);
  int tile = ti_.first;
  bool have = tile < ti_.last;
  if (have) prefetch(tile);

  if (st.rtr_stop || (!first && st.tcg_done)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      store_state(sout, st);
      publish_progress(hflag, gen, st);
    }
    return;
  }
  double alpha, tau;
  const int mode = tcg_update_prologue(st, pin, nb_in, first, red, alpha, tau, &praw);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    store_state(sout, st);
    tcg_store_coef<DEF>(coef, st, mode, alpha, tau);
    publish_progress(hflag, gen, st);
  }

  DPGO_STAMP(1, 2);
  double part[2] = {0.0, 0.0};
  while (have) {
    const size_t base = (size_t)p0 * GEO::T;
    [[maybe_unused]] dbl2* eta2 = reinterpret_cast<dbl2*>(eta + base);
    if (mode == 1) {  // workgroup-uniform: eta += tau * delta, then tCG stops
      // (r += tau * H delta with it: r = g + H eta holds at every exit of tCG, which is what the rho test reads, k_retract)
      dbl2* r2 = reinterpret_cast<dbl2*>(r + base);
#pragma unroll
      for (int it = 0; it < SPN::NIT; ++it) {
        const int pc = lane + 64 * it;
        if (2 * pc < valid) {
          dbl2 rr = rv[it];
          if constexpr (!DEF) {
            dbl2 e = ev[it];
            e.x = fma(tau, dv[it].x, e.x);
            e.y = fma(tau, dv[it].y, e.y);
            eta2[pc] = e;
          }
          rr.x = fma(tau, hv[it].x, rr.x);
          rr.y = fma(tau, hv[it].y, rr.y);
          r2[pc] = rr;
        }
      }
      request_next(tile, have);
    } else {
      dbl2* r2 = reinterpret_cast<dbl2*>(r + base);
#pragma unroll
      for (int it = 0; it < SPN::NIT; ++it) {
        const int pc = lane + 64 * it;
        if (2 * pc < valid) {
          if (!ml_mode) reinterpret_cast<dbl2*>(ys)[pc] = xv[it];
          dbl2 rr = rv[it];
          if (mode == 2) {
            if constexpr (!DEF) {
              dbl2 zero;
              zero.x = 0.0;
              zero.y = 0.0;
              eta2[pc] = zero;
            }
          } else {
            if constexpr (!DEF) {
              dbl2 e = ev[it];
              e.x = fma(alpha, dv[it].x, e.x);
              e.y = fma(alpha, dv[it].y, e.y);
              eta2[pc] = e;
            }
            rr.x = fma(alpha, hv[it].x, rr.x);
            rr.y = fma(alpha, hv[it].y, rr.y);
          }
          r2[pc] = rr;
          reinterpret_cast<dbl2*>(rs)[pc] = rr;
          part[0] = fma(rr.x, rr.x, part[0]);
          part[0] = fma(rr.y, rr.y, part[0]);
        }
      }
      request_next(tile, have);
      wave_sync();
      double zz[R];
      if (ok) {
        const double* rt = rs + L.g * GEO::T;
        if (dinv) {
          jacobi_col<D, R>(rt, drow, zz);
        } else {
#pragma unroll
          for (int a = 0; a < R; ++a) zz[a] = rt[L.c * R + a];
        }
        store_col<R>(zs + L.g * GEO::T + L.c * R, zz);
      }
      wave_sync();
      if (ok) {
        double out[R], sdummy[D];
        if (ml_mode) {
#pragma unroll
          for (int a = 0; a < R; ++a) out[a] = ml_omega * zz[a];
        } else {
          proj_col<D, R>(ys + L.g * GEO::T, zs + L.g * GEO::T, L.c, zz, out, sdummy);
        }
        const double* rt = rs + L.g * GEO::T + L.c * R;
#pragma unroll
        for (int a = 0; a < R; ++a) part[1] = fma(out[a], rt[a], part[1]);
        store_col<R>(os + L.g * GEO::T + L.c * R, out);
      }
      wave_sync();
      if (z32) {
        float2* zf = reinterpret_cast<float2*>(z32 + base);
#pragma unroll
        for (int it = 0; it < SPN::NIT; ++it) {
          const int pc = lane + 64 * it;
          if (2 * pc < valid) {
            const dbl2 v = reinterpret_cast<const dbl2*>(os)[pc];
            zf[pc] = make_float2((float)v.x, (float)v.y);
          }
        }
      } else {
        dbl2* z2 = reinterpret_cast<dbl2*>(z + base);
#pragma unroll
        for (int it = 0; it < SPN::NIT; ++it) {
          const int pc = lane + 64 * it;
          if (2 * pc < valid) z2[pc] = reinterpret_cast<const dbl2*>(os)[pc];
        }
      }
      wave_sync();
    }
    DPGO_STAMP(1, 5);
    if constexpr (PIPE) {
      if (have) {
        p0 = p0_n;
        valid = valid_n;
        i = i_n;
        ok = ok_n;
#pragma unroll
        for (int k = 0; k < GEO::B; ++k) drow[k] = drow_n[k];
      }
    } else {
      tile += ti_.step;
      have = tile < ti_.last;
      if (have) prefetch(tile);
    }
  }
  if (mode != 1) store_partials<2>(part, pout, red);
  DPGO_STAMP(1, 6);
  DPGO_COMMIT(1);
}

// ================================================================ K7a: tCG residual / iterate update
// ROPTLIB SolversTR::tCG_TR, first half of one inner iteration (and, with first = 1, its
// initialisation r = g, eta = 0, z = P(r)):
//   d_Hd (from k_hess partials) -> alpha, e_Pe';  boundary / negative curvature -> eta += tau*delta, r += tau*Hd, stop
//   else eta += alpha*delta; r += alpha*Hd; z = P(r);  partials: [0] <r,r>  [1] <z,r>
template <int D, int R, int DEF = 0>
__global__ __launch_bounds__(kBlock, DPGO_LB_UPDATE) void k_tcg_update(const double* __restrict__ X, const double* __restrict__ g,
                                                       const double* __restrict__ dinv,
                                                       const double* __restrict__ delta,
                                                       const double* __restrict__ Hd, double* __restrict__ eta,
                                                       double* __restrict__ r, double* __restrict__ z,
                                                       const double* __restrict__ pin, int nb_in,
                                                       double* __restrict__ pout, const DevState* __restrict__ sin,
                                                       DevState* __restrict__ sout, int first, int n,
                                                       unsigned long long* hflag, unsigned gen, double ml_omega,
                                                       double* __restrict__ coef) {
  // generic layout (odd tile size); even tile sizes run k_tcg_update_span
  using GEO = Geo<D, R>;
  __shared__ __attribute__((aligned(16))) double sm[kWaves][3][GEO::G][GEO::T];
  __shared__ double red[kWaves * kNP];
  DevState st;
  load_state(st, sin);
  gen = state_gen(st, gen);
  if (st.rtr_stop || (!first && st.tcg_done)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      store_state(sout, st);
      publish_progress(hflag, gen, st);
    }
    return;
  }
  double alpha, tau;
  const int mode = tcg_update_prologue(st, pin, nb_in, first, red, alpha, tau);  // 0: step, 1: boundary step, 2: init
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    store_state(sout, st);
    tcg_store_coef<DEF>(coef, st, mode, alpha, tau);
    publish_progress(hflag, gen, st);
  }

  const LaneId L = lane_id<D>();
  const int ntiles = (n + GEO::P - 1) / GEO::P;
  double part[2] = {0.0, 0.0};
  const TileIter ti_ = tile_iter(ntiles);
  for (int tile = ti_.first; tile < ti_.last; tile += ti_.step) {
    const int i = tile * GEO::P + L.wave * GEO::G + L.g;
    const bool ok = (L.g < GEO::G) && (i < n);
    const size_t off = (size_t)i * GEO::T + L.c * R;
    if (mode == 1) {  // workgroup-uniform
      if (ok) {
        // (r += tau * H delta with it: r = g + H eta holds at every exit of tCG, which is what the rho test reads)
        double hd[R], rr[R];
        if constexpr (!DEF) {
          double e[R], dl[R];
          load_col<R>(eta + off, e);
          load_col<R>(delta + off, dl);
#pragma unroll
          for (int a = 0; a < R; ++a) e[a] = fma(tau, dl[a], e[a]);
          store_col<R>(eta + off, e);
        }
        load_col<R>(Hd + off, hd);
        load_col<R>(r + off, rr);
#pragma unroll
        for (int a = 0; a < R; ++a) rr[a] = fma(tau, hd[a], rr[a]);
        store_col<R>(r + off, rr);
      }
      continue;
    }
    double* ys = ok ? &sm[L.wave][0][L.g][0] : nullptr;
    double* rs = ok ? &sm[L.wave][1][L.g][0] : nullptr;
    double* zs = ok ? &sm[L.wave][2][L.g][0] : nullptr;
    double rr[R], x[R], zz[R], drow[GEO::B];
    if (ok) {
      // all of this pose's loads are issued back to back (independent addresses)
      load_col<R>(X + off, x);
      if (dinv) {
#pragma unroll
        for (int k = 0; k < GEO::B; ++k) drow[k] = dinv[(size_t)i * GEO::BB + L.c * GEO::B + k];
      }
      if (mode == 2) {
        load_col<R>(g + off, rr);
        if constexpr (!DEF) {
          double e[R];
#pragma unroll
          for (int a = 0; a < R; ++a) e[a] = 0.0;
          store_col<R>(eta + off, e);
        }
      } else {
        double hd[R];
        if constexpr (!DEF) {
          double e[R], dl[R];
          load_col<R>(eta + off, e);
          load_col<R>(delta + off, dl);
#pragma unroll
          for (int a = 0; a < R; ++a) e[a] = fma(alpha, dl[a], e[a]);
          store_col<R>(eta + off, e);
        }
        load_col<R>(Hd + off, hd);
        load_col<R>(r + off, rr);
#pragma unroll
        for (int a = 0; a < R; ++a) rr[a] = fma(alpha, hd[a], rr[a]);
      }
      store_col<R>(r + off, rr);
#pragma unroll
      for (int a = 0; a < R; ++a) part[0] = fma(rr[a], rr[a], part[0]);
      store_col<R>(ys + L.c * R, x);
      store_col<R>(rs + L.c * R, rr);
    }
    wave_sync();
    if (ok) {
      if (dinv) {
        jacobi_col<D, R>(rs, drow, zz);
      } else {
#pragma unroll
        for (int a = 0; a < R; ++a) zz[a] = rr[a];
      }
      store_col<R>(zs + L.c * R, zz);
    }
    wave_sync();
    if (ok) {
      double out[R], s[D];
      if (ml_omega > 0.0) {
#pragma unroll
        for (int a = 0; a < R; ++a) out[a] = ml_omega * zz[a];
      } else {
        proj_col<D, R>(ys, zs, L.c, zz, out, s);
      }
#pragma unroll
      for (int a = 0; a < R; ++a) part[1] = fma(out[a], rr[a], part[1]);
      store_col<R>(z + off, out);
    }
    wave_sync();
  }
  if (mode != 1) store_partials<2>(part, pout, red);
}
